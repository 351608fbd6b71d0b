"""Model kernels against a float64 oracle of what they are meant to compute.

The oracle (part 1) is plain numpy, straight-line, and shares nothing with
the kernels or with ``MyCNNEngine``: conv1 -> tanh -> pool -> conv2 -> tanh
-> pool, then the two-layer batch-as-time LSTM, the head and the age gate.

The *exact* inputs (part 2) make conv1 a sum of multiples of 1/64 that
never exceeds 12.5 in magnitude: windows of +-1, conv1 weights nonzero
multiples of 1/64 in [-8/64, 8/64], biases multiples of 1/64 in the same
range. All are exact in bf16, and every partial sum is exact in fp32, so the
MFMA accumulation order, the VALU two-accumulator order and float64 agree
bit for bit before the first tanh: a misplaced element cannot hide in
rounding. What is left is ``tanhf_`` and the 21-term fp32 conv2 chain, which
is why the fp32 conv path's tolerance (rtol 2e-5, atol 2e-6) applies to every
conv kernel on these inputs. The CPU tests make those claims, and the claim
that a wrong tap, a wrong channel or a wrong reduction order moves the
features by more than 100 x that tolerance, part of the suite.

Figures measured on an MI355X are in docs/KERNELS.md ("Exact model tests").
"""

import copy

import numpy as np
import pytest
import torch

from tskd_amd.models import build_model

VARIANTS = ("MyCNN5", "MyCNN2", "MyCNN3", "MyCNN4")
TLAST_VARIANTS = ("MyCNN5", "MyCNN4")        # even channel counts
FEAT_RTOL, FEAT_ATOL = 2e-5, 2e-6            # test_conv_features_parity
LOGIT_RTOL, LOGIT_ATOL = 2e-4, 2e-5          # test_fp32_parity
NWIN = 64                                    # distinct exact windows
PERIOD = 61                                  # pattern length past the grid cap
GRID_CAP = 8192                              # blocks, every launcher
_SEED = {"MyCNN5": 505, "MyCNN2": 202, "MyCNN3": 303, "MyCNN4": 404}


# --------------------------------------------------------------------------
# 1. The oracle
# --------------------------------------------------------------------------
def bf16_round(a):
    """float32 array -> the float32 values of its bf16 rounding (round to
    nearest, ties to even; NaN stays a quiet NaN), in integer arithmetic."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = u.astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u >> 16) | 0x40, r)
    return (r << 16).astype(np.uint32).view(np.float32)


def _as_np(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu()
        if x.dtype == torch.bfloat16:
            x = x.float()
        x = x.numpy()
    return np.asarray(x)


def _conv1(w1, b1, x):
    """(n, 4, C1) float64 pre-activations; w1 (4, CIN, K1), b1 (4,),
    x (n, CIN, L), all float64. Reduction over (i, k), k the time tap."""
    n, cin, length = x.shape
    k1 = w1.shape[2]
    c1 = length - k1 + 1
    pre = np.tile(b1[None, :, None], (n, 1, c1))
    for i in range(cin):
        for k in range(k1):
            pre = pre + w1[None, :, i, k, None] * x[:, i, None, k:k + c1]
    return pre


def _pool(a, pk, ps):
    p = (a.shape[-1] - pk) // ps + 1
    span = (p - 1) * ps + 1
    out = a[..., 0:span:ps]
    for k in range(1, pk):
        out = np.maximum(out, a[..., k:k + span:ps])
    return out


def _features(w1, b1, w2, b2, x, pk, ps):
    """conv1 -> tanh -> pool -> conv2 -> tanh -> pool on float64 arrays:
    w2 (4, 5), b2 scalar; returns (n, LIN)."""
    p1 = _pool(np.tanh(_conv1(w1, b1, x)), pk, ps)      # (n, 4, P1)
    c2 = p1.shape[-1] - 5 + 1
    pre2 = np.full((x.shape[0], c2), b2, dtype=np.float64)
    for c in range(4):
        for k in range(5):
            pre2 = pre2 + w2[c, k] * p1[:, c, k:k + c2]
    return _pool(np.tanh(pre2), pk, ps)


def _conv_params(model, bf16_path):
    w1 = _as_np(model.conv1.weight).astype(np.float32)
    if bf16_path:
        w1 = bf16_round(w1)
    return (w1.astype(np.float64),
            _as_np(model.conv1.bias).astype(np.float64),
            _as_np(model.conv2.weight).astype(np.float64).reshape(4, 5),
            float(_as_np(model.conv2.bias).astype(np.float64)[0]))


def _windows64(x, bf16_path):
    x = _as_np(x)
    x = x.reshape(-1, x.shape[-2], x.shape[-1])
    if bf16_path:
        x = bf16_round(x.astype(np.float32))
    return x.astype(np.float64)


def oracle_features(model, x, bf16_path):
    """(..., CIN, 120) windows -> (..., LIN) float64 features. With
    ``bf16_path`` the windows and conv1.weight are first rounded to bf16, as
    the MFMA kernels and pack_conv1_mfma_bfrags see them; bias, conv2 and all
    after are the fp32 parameters taken to float64."""
    lead = tuple(_as_np(x).shape[:-2])
    w1, b1, w2, b2 = _conv_params(model, bf16_path)
    f = _features(w1, b1, w2, b2, _windows64(x, bf16_path),
                  int(model.POOL_K), int(model.POOL_S))
    return f.reshape(lead + (f.shape[-1],))


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def oracle_logits(model, feats, age, sigmoid):
    """(S, N, LIN) or (N, LIN) float64 features -> (S, N) or (N,) logits:
    two-layer LSTM scanned over N from zero state (gate rows i, f, g, o;
    bias = b_ih + b_hh), Linear(16, 1), times relu(age * eps + 1), optional
    sigmoid. ``age`` is None (gate 1) or shaped like the result."""
    f = np.asarray(_as_np(feats), dtype=np.float64)
    squeeze = f.ndim == 2
    if squeeze:
        f = f[None]
    S, N, _ = f.shape
    sd = {k: _as_np(v).astype(np.float64)
          for k, v in model.state_dict().items()}
    wih = [sd["lstm.weight_ih_l0"], sd["lstm.weight_ih_l1"]]
    whh = [sd["lstm.weight_hh_l0"], sd["lstm.weight_hh_l1"]]
    b = [sd["lstm.bias_ih_l0"] + sd["lstm.bias_hh_l0"],
         sd["lstm.bias_ih_l1"] + sd["lstm.bias_hh_l1"]]
    wo, bo = sd["out.weight"][0], sd["out.bias"][0]
    h = [np.zeros((S, 16)), np.zeros((S, 16))]
    c = [np.zeros((S, 16)), np.zeros((S, 16))]
    out = np.empty((S, N), dtype=np.float64)
    for t in range(N):
        inp = f[:, t]
        for l in range(2):
            g = inp @ wih[l].T + h[l] @ whh[l].T + b[l]
            gi, gf = _sig(g[:, 0:16]), _sig(g[:, 16:32])
            gg, go = np.tanh(g[:, 32:48]), _sig(g[:, 48:64])
            c[l] = gf * c[l] + gi * gg
            h[l] = go * np.tanh(c[l])
            inp = h[l]
        out[:, t] = h[1] @ wo + bo
    if age is not None:
        a = np.asarray(_as_np(age), dtype=np.float64).reshape(S, N)
        out = out * np.maximum(a * float(model.AGE_EPS) + 1.0, 0.0)
    if sigmoid:
        out = _sig(out)
    return out[0] if squeeze else out


# --------------------------------------------------------------------------
# 2. The exact inputs
# --------------------------------------------------------------------------
def exact_model(name, age_eps=None):
    """``name`` at its seeded default initialisation, conv1 replaced by
    nonzero multiples of 1/64 in [-8/64, 8/64] (bias: multiples, zero
    allowed). Magnitudes are 1..6, which keeps the 100-term MyCNN5 sums
    out of tanh's saturation, except the corner taps (first and last
    channel, first and last time tap), which are +-8/64 so that losing one
    is unmistakable."""
    torch.manual_seed(_SEED[name])
    m = build_model(name).eval()
    rng = np.random.default_rng(_SEED[name])
    shape = tuple(m.conv1.weight.shape)
    w = rng.integers(1, 7, size=shape) * rng.choice([-1, 1], size=shape)
    for i in (0, shape[1] - 1):
        for k in (0, shape[2] - 1):
            w[:, i, k] = np.sign(w[:, i, k]) * 8
    bias = rng.integers(-8, 9, size=4)
    with torch.no_grad():
        m.conv1.weight.copy_(torch.from_numpy(w / 64.0))
        m.conv1.bias.copy_(torch.from_numpy(bias / 64.0))
    if age_eps is not None:
        m.AGE_EPS = age_eps
    return m


def exact_windows(cin, n=NWIN, length=120, seed=0):
    """(n, cin, length) float32 of +-1, never 0."""
    rng = np.random.default_rng(1000 + 10 * cin + seed)
    return rng.choice(np.float32([-1.0, 1.0]), size=(n, cin, length))


_cache = {}


def exact_case(name):
    """(model, windows (NWIN, CIN, 120) float32, oracle features float64):
    computed once per variant and left unchanged."""
    if name not in _cache:
        m = exact_model(name)
        x = exact_windows(int(m.IN_CHANNELS))
        f = oracle_features(m, x, bf16_path=True)
        x.setflags(write=False)
        f.setflags(write=False)
        _cache[name] = (m, x, f)
    return _cache[name]


def feat_tol(ref, scale=1.0):
    return scale * (FEAT_ATOL + FEAT_RTOL * np.abs(ref))


# --------------------------------------------------------------------------
# CPU: the oracle checks itself, the construction's claims hold
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", VARIANTS)
def test_oracle_matches_double_model(name):
    torch.manual_seed(7)
    m = build_model(name).eval()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(5, m.IN_CHANNELS, 120, generator=g)
    age = torch.tensor([35.0, 52.5, 61.0, 70.0, 88.0])
    md = copy.deepcopy(m).double()
    with torch.no_grad():
        fr = md.pool(torch.tanh(md.conv2(md.pool(torch.tanh(
            md.conv1(x.double())))))).view(5, -1).numpy()
        lr = md(x.double(), age.double()).numpy()
    f = oracle_features(m, x, bf16_path=False)
    assert f.shape == fr.shape == (5, m.LSTM_IN)
    assert np.abs(f - fr).max() <= 1e-12
    for sig in (False, True):
        ref = 1.0 / (1.0 + np.exp(-lr)) if sig else lr
        got = oracle_logits(m, f, age, sig)
        assert got.shape == (5,)
        assert np.abs(got - ref).max() <= 1e-12
    # batched form: S independent scans (BLAS may order a batched sum
    # differently, hence not bit for bit)
    two = oracle_logits(m, np.stack([f, f[::-1]]), None, False)
    for row, fs in zip(two, (f, f[::-1])):
        assert np.abs(row - oracle_logits(m, fs, None, False)).max() <= 1e-14


def test_bf16_round_matches_torch():
    bits = np.array([
        0x3F800000, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001,  # ties
        0x3F80FFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,  # -> inf
        0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00018000,  # denorm
        0x00007FFF, 0x007FFFFF, 0x807F8000, 0x00800000, 0x0000FFFF,
        0x7F800000, 0xFF800000, 0x42F08000, 0xC2F18000, 0x3DCCCCCD,  # +-inf
    ], dtype=np.uint32)
    rng = np.random.default_rng(3)
    rnd = rng.integers(0, 2 ** 32, size=4096, dtype=np.uint64)
    rnd = rnd.astype(np.uint32)
    rnd = rnd[(rnd & 0x7FFFFFFF) <= 0x7F800000]          # no NaN patterns
    a = np.concatenate([bits, rnd]).view(np.float32)
    got = bf16_round(a)
    ref = torch.from_numpy(a.copy()).to(torch.bfloat16).float().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    nan = bf16_round(np.array([np.nan, -np.nan], dtype=np.float32))
    assert np.isnan(nan).all()


@pytest.mark.parametrize("name", VARIANTS)
def test_exact_construction(name):
    """The inputs are what the module says: +-1 windows, conv1 parameters
    multiples of 1/64, all bf16-exact, tanh not saturated."""
    m, x, _ = exact_case(name)
    w = _as_np(m.conv1.weight)
    b = _as_np(m.conv1.bias)
    assert set(np.unique(x)) == {-1.0, 1.0}
    for a in (w * 64, b * 64):
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 8
    assert (w != 0).all()
    for a in (w, b, x):
        assert np.array_equal(bf16_round(a), a)
    w1, b1, _, _ = _conv_params(m, True)
    pre = np.abs(_conv1(w1, b1, x.astype(np.float64)))
    print(f"[exact] {name}: max |pre-activation| = {pre.max():.3f}, "
          f"share above 2 = {(pre > 2).mean():.4f}")
    assert pre.max() < 4.0          # tanh' > 1.3e-3: every output resolves
    assert (pre > 2).mean() < 0.01


@pytest.mark.parametrize("name", VARIANTS)
def test_conv1_exact_under_permuted_fp32_summation(name):
    m, x, _ = exact_case(name)
    x = x[:8]
    w1, b1, _, _ = _conv_params(m, True)
    ref = _conv1(w1, b1, x.astype(np.float64))            # (8, 4, C1)
    cin, k1 = w1.shape[1], w1.shape[2]
    c1 = ref.shape[-1]
    terms = [np.float32(w1[None, :, i, k, None]) *
             x[:, i, None, k:k + c1] for i in range(cin) for k in range(k1)]
    rng = np.random.default_rng(11)
    for _ in range(3):
        acc = np.broadcast_to(np.float32(b1)[None, :, None], ref.shape)
        order = rng.permutation(len(terms))
        half = len(order) // 2
        # two fp32 accumulators joined at the end, then one chain
        a0 = acc.copy()
        a1 = np.zeros_like(a0)
        for p in order[:half]:
            a0 = (a0 + terms[p]).astype(np.float32)
        for p in order[half:]:
            a1 = (a1 + terms[p]).astype(np.float32)
        assert a0.dtype == np.float32
        assert np.array_equal((a0 + a1).astype(np.float64), ref)
        one = acc.copy()
        for p in order:
            one = (one + terms[p]).astype(np.float32)
        assert np.array_equal(one.astype(np.float64), ref)


def _moved(f, ref):
    """Per feature: moved by more than 100 x the GPU tolerance."""
    return np.abs(f - ref) > feat_tol(ref, 100.0)


@pytest.mark.parametrize("name", VARIANTS)
def test_mutation_zeroed_corner_tap(name):
    m, x, ref = exact_case(name)
    w1, b1, w2, b2 = _conv_params(m, True)
    x64 = x.astype(np.float64)
    pk, ps = int(m.POOL_K), int(m.POOL_S)
    cin, k1 = w1.shape[1], w1.shape[2]
    for o in range(4):
        for i in (0, cin - 1):
            for k in (0, k1 - 1):
                wm = w1.copy()
                wm[o, i, k] = 0.0
                share = _moved(_features(wm, b1, w2, b2, x64, pk, ps),
                               ref).mean()
                assert share >= 0.90, (o, i, k, share)


@pytest.mark.parametrize("name", VARIANTS)
def test_mutation_flipped_corner_sample(name):
    m, x, ref = exact_case(name)
    w1, b1, w2, b2 = _conv_params(m, True)
    pk, ps = int(m.POOL_K), int(m.POOL_S)
    cin = w1.shape[1]
    for c, t in ((cin - 1, 119), (0, 0)):
        xm = x.astype(np.float64)
        xm[:, c, t] *= -1.0
        moved = _moved(_features(w1, b1, w2, b2, xm, pk, ps), ref)
        nwin = int(moved.any(axis=1).sum())
        # the maxpool hides the flip in the other windows: hence 64 of them
        assert nwin >= 8, (c, t, nwin)


@pytest.mark.parametrize("name", VARIANTS)
def test_mutation_wrong_channel_or_reduction_order(name):
    m, x, ref = exact_case(name)
    w1, b1, w2, b2 = _conv_params(m, True)
    pk, ps = int(m.POOL_K), int(m.POOL_S)
    cin, k1 = w1.shape[1], w1.shape[2]
    x64 = x.astype(np.float64)
    for a, b in ((0, 1), (0, cin - 1), (cin - 2, cin - 1)):
        xm = x64.copy()
        xm[:, [a, b]] = xm[:, [b, a]]
        moved = _moved(_features(w1, b1, w2, b2, xm, pk, ps), ref)
        assert moved.mean() >= 0.5, (a, b, moved.mean())
    # the flat weight row read as [k][i] instead of [i][k]
    wt = w1.reshape(4, k1, cin).transpose(0, 2, 1)
    moved = _moved(_features(wt, b1, w2, b2, x64, pk, ps), ref)
    assert moved.mean() >= 0.5, moved.mean()


# --------------------------------------------------------------------------
# GPU helpers
# --------------------------------------------------------------------------
KERNELS = ("fp32", "staged", "tlast")


def kernel_cases(variants_fp=VARIANTS):
    return [(k, v) for k in KERNELS
            for v in (TLAST_VARIANTS if k == "tlast" else variants_fp)]


_engines = {}


def engine_for(name, model=None, key=None):
    from tskd_amd.ops import MyCNNEngine
    key = key or name
    if key not in _engines:
        _engines[key] = MyCNNEngine(model or exact_case(name)[0],
                                    device="cuda")
    return _engines[key]


def dev(a):
    """Device copy of a host array (the cached exact arrays are read-only)."""
    return torch.from_numpy(np.array(a)).cuda()


def conv_input(kernel, xd, tagged=True):
    """Device windows (n, CIN, 120) fp32 -> the tensor ``kernel`` takes:
    fp32 (n, CIN, 120), bf16 (n, CIN, 120) or bf16 time-last (n, 120, CIN),
    the last in an alloc_windows buffer unless ``tagged`` is False."""
    from tskd_amd.ops import alloc_windows
    if kernel == "fp32":
        return xd.clone()
    if kernel == "staged":
        return xd.to(torch.bfloat16)
    xt = xd.transpose(-1, -2).to(torch.bfloat16).contiguous()
    if not tagged:
        return xt
    n, cin = xd.shape[0], xd.shape[1]
    buf = alloc_windows(1, n, cin, timelast=True, dtype=torch.bfloat16)
    buf.copy_(xt.reshape(buf.shape))
    return buf


def run_conv(eng, kernel, xin):
    """conv_features on what conv_input made -> (n, LIN) fp32 on the host."""
    f = eng.conv_features(xin)
    torch.cuda.synchronize()
    return f.reshape(-1, f.shape[-1]).cpu()


def assert_feats(got, ref, what):
    got = got.double().numpy()
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    bad = err > feat_tol(ref)
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} of {bad.size} features off, max |err| "
        f"{err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}")
    return float(err.max())


def assert_logits(got, ref, what):
    got = got.detach().cpu().double().numpy().reshape(ref.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    bad = err > LOGIT_ATOL + LOGIT_RTOL * np.abs(ref)
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} of {bad.size} off, max |err| "
        f"{err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}")
    return float(err.max())


# --------------------------------------------------------------------------
# 3. GPU: every conv kernel, and the fused tail, on the exact inputs
# --------------------------------------------------------------------------
@pytest.mark.gpu
class TestExactConv:
    SNS = (1, 2, 7, 8, 9, 64)   # lone window, one pair, odd pair tail, one
    # workgroup of pairs, a wave's second pass, the whole set

    @pytest.mark.parametrize("kernel,name", kernel_cases())
    def test_conv_kernel_vs_oracle(self, kernel, name):
        _, x, ref = exact_case(name)
        eng = engine_for(name)
        xd = dev(x)
        worst = 0.0
        for sn in self.SNS:
            got = run_conv(eng, kernel, conv_input(kernel, xd[:sn]))
            assert got.shape == (sn, ref.shape[1])
            worst = max(worst, assert_feats(got, ref[:sn],
                                            f"{kernel} {name} SN={sn}"))
        print(f"[exact conv] {kernel} {name}: max |err| = {worst:.3e}")

    @pytest.mark.parametrize("name", TLAST_VARIANTS)
    def test_tlast_untagged_tensor(self, name):
        """A time-last tensor without the slack tag is copied into a padded
        buffer by the wrapper and scores the same."""
        _, x, ref = exact_case(name)
        eng = engine_for(name)
        xin = conv_input("tlast", dev(x)[:9],
                         tagged=False)
        assert not getattr(xin, "_tskd_slack", False)
        worst = assert_feats(run_conv(eng, "tlast", xin), ref[:9],
                             f"tlast untagged {name}")
        print(f"[exact conv] tlast untagged {name}: max |err| = {worst:.3e}")


RING_G = 192


def ring_engine(S, G, pattern):
    """StreamEngine whose ``proc`` ring rows repeat ``pattern`` (P, C, G);
    returns (engine, stream -> pattern row index)."""
    from tskd_amd.engine import StreamEngine
    C = pattern.shape[1]
    se = StreamEngine(S, C, ring_grid=G, fs=25.0, device="cuda")
    idx = torch.arange(S, device="cuda") % pattern.shape[0]
    se.proc.copy_(torch.from_numpy(pattern).cuda()[idx])
    return se, idx.cpu().numpy()


def ring_windows(pattern, G, nproc):
    """Host read of the window ending at grid point ``nproc``: (P, C, 120)."""
    slots = np.arange(nproc - 120, nproc) % G
    return pattern[:, :, slots]


def stream_ages(S):
    """A different age per stream, far enough apart that a neighbour's age
    moves a MyCNN4 logit (eps 1e-4) by per cent."""
    s = np.arange(S, dtype=np.float32)
    return (30.0 + 700.0 * s * np.where(s % 2 == 0, 1.0, -1.0)).reshape(S, 1)


@pytest.mark.gpu
class TestExactFusedTail:
    @pytest.mark.parametrize("S", [1, 3, 9])
    @pytest.mark.parametrize("name", TLAST_VARIANTS)
    def test_fused_and_unfused_vs_oracle(self, name, S):
        m, _, _ = exact_case(name)
        eng = engine_for(name)
        pattern = exact_windows(10, n=S, length=RING_G, seed=S)
        se, _ = ring_engine(S, RING_G, pattern)
        age = stream_ages(S)
        age_d = torch.from_numpy(age).cuda()
        worst = {"fused": 0.0, "unfused": 0.0}
        # first full window, one ending at the ring end, one across the wrap
        for nproc in (120, 192, 200):
            se.nproc = nproc
            feats = oracle_features(m, ring_windows(pattern, RING_G, nproc),
                                    bf16_path=True).reshape(S, 1, -1)
            w = se.windows(batch=1, stride=12, dtype=torch.bfloat16,
                           timelast=True)
            for a_np, a_d in ((None, None), (age, age_d)):
                for sig in (False, True):
                    ref = oracle_logits(m, feats, a_np, sig)
                    what = f"{name} S={S} nproc={nproc} " \
                           f"age={a_np is not None} sigmoid={sig}"
                    got = se.score_latest(eng, a_d, apply_sigmoid=sig)
                    torch.cuda.synchronize()
                    assert got.shape == (S, 1)
                    worst["fused"] = max(worst["fused"], assert_logits(
                        got, ref, "score_latest " + what))
                    got = eng.forward(w, a_d, apply_sigmoid=sig)
                    torch.cuda.synchronize()
                    worst["unfused"] = max(worst["unfused"], assert_logits(
                        got, ref, "forward(windows) " + what))
        print(f"[exact tail] {name} S={S}: max |err| fused "
              f"{worst['fused']:.3e}, unfused {worst['unfused']:.3e}")


# --------------------------------------------------------------------------
# 4. GPU: general values, tolerance derived from the oracle's own quantities
# --------------------------------------------------------------------------
PHYS_OFFSETS = (80.0, 97.0, 120.0, 36.6, 18.0, 75.0, 60.0, 95.0, 12.0, 5.0)
# Default-initialisation seeds at which the physiological windows drive
# conv1 channels past +-44.4 on BOTH sides: tanhf_ is 2 / (1 + __expf(-2x))
# - 1, whose exp overflows to inf for x < -44.4 and underflows to 0 on the
# other side. The test asserts that this holds (a condition on the inputs).
# Found on the CPU, from the oracle's conv1 alone and before any kernel ran:
# the first of the seeds _SEED[name] + 1 + 1000 * k, k = 0, 1, ..., whose
# pre-activations pass both edges with some margin (most seeds pass one).
GENERAL_SEED = {"MyCNN5": 2506, "MyCNN2": 9203, "MyCNN3": 304, "MyCNN4": 7405}
EXP_EDGE = 44.4


def general_windows(kind, cin, n=16):
    g = torch.Generator().manual_seed(40 + cin + len(kind))
    x = torch.randn(n, cin, 120, generator=g)
    if kind == "randn2":
        x = x * 2.0
    else:                       # physiological scale: tanh saturates
        x = x + torch.tensor(PHYS_OFFSETS[:cin]).reshape(1, cin, 1)
    return x.to(torch.bfloat16).float().numpy()


def derived_feature_bound(model, x, bf16_path):
    """First-order bound on the features' error from fp32 summation of conv1
    in any order: (KK + 1) * 2^-24 * max sum |w x| over conv1 outputs,
    through the 1-Lipschitz tanh and pools, times sum |w2| through conv2,
    plus the exact-input atol for what comes after conv1."""
    w1, _, w2, _ = _conv_params(model, bf16_path)
    kk = w1.shape[1] * w1.shape[2]
    mag = _conv1(np.abs(w1), np.zeros(4), np.abs(_windows64(x, bf16_path)))
    return (kk + 1) * 2.0 ** -24 * mag.max() * np.abs(w2).sum() + FEAT_ATOL


@pytest.mark.gpu
class TestGeneralValues:
    @pytest.mark.parametrize("kind", ["randn2", "phys"])
    @pytest.mark.parametrize("kernel,name", kernel_cases())
    def test_conv_kernel_within_derived_bound(self, kernel, name, kind):
        torch.manual_seed(GENERAL_SEED[name])
        m = build_model(name).eval()        # default initialisation
        eng = engine_for(name, m, key=("default", name))
        x = general_windows(kind, int(m.IN_CHANNELS))
        # the fp32 kernel multiplies by the unrounded fp32 conv1 weights;
        # the windows hold bf16-exact values for every kernel
        bf16_path = kernel != "fp32"
        ref = oracle_features(m, x, bf16_path)
        bound = derived_feature_bound(m, x, bf16_path)
        got = run_conv(eng, kernel, conv_input(
            kernel, dev(x))).double().numpy()
        assert np.isfinite(got).all()
        err = np.abs(got - ref).max()
        w1, b1, _, _ = _conv_params(m, bf16_path)
        pre = _conv1(w1, b1, _windows64(x, bf16_path))
        lo, hi = (pre < -EXP_EDGE).mean(), (pre > EXP_EDGE).mean()
        print(f"[general] {kernel} {name} {kind}: max |err| = {err:.3e}, "
              f"bound = {bound:.3e}, ratio = {err / bound:.4f}; conv1 "
              f"pre-activations {pre.min():.1f} .. {pre.max():.1f}, share "
              f"below -{EXP_EDGE} = {lo:.2f}, above = {hi:.2f}")
        if kind == "phys":
            assert lo > 0.1 and hi > 0.1    # tanhf_'s exp leaves fp32 range
        assert err <= 2.0 * bound
        assert (np.abs(got) <= 1.0).all()


# --------------------------------------------------------------------------
# 5. GPU: lstm_head_kernel on its own
# --------------------------------------------------------------------------
HEAD_VARIANTS = ("MyCNN5", "MyCNN3")          # LIN = 25 and 27
HEAD_NS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 97)
HEAD_SS = (1, 4, 5, 9)
CLAMP_AGE = -20000.0                          # 1e-4 * age + 1 = -1 -> gate 0


def head_model(name):
    """Default-initialised ``name`` under MyCNN4's AGE_EPS, so age counts."""
    torch.manual_seed(_SEED[name] + 2)
    m = build_model(name).eval()
    m.AGE_EPS = 1e-4
    return m


def head_inputs(lin, S, N):
    rng = np.random.default_rng(S * 1000 + N)
    feats = rng.uniform(-1.0, 1.0, size=(S, N, lin)).astype(np.float32)
    age = rng.uniform(-4000.0, 4000.0, size=(S, N)).astype(np.float32)
    return feats, age


@pytest.mark.gpu
class TestLstmHead:
    @pytest.mark.parametrize("N", HEAD_NS)
    @pytest.mark.parametrize("name", HEAD_VARIANTS)
    def test_scan_vs_oracle(self, name, N):
        m = head_model(name)
        eng = engine_for(name, m, key=("head", name))
        assert eng.age_eps == 1e-4
        worst = 0.0
        for S in HEAD_SS:
            feats, age = head_inputs(eng.feat_len, S, N)
            fd = torch.from_numpy(feats).cuda()
            clamp = age.copy()
            clamp[:, ::2] = CLAMP_AGE         # every other step is gated off
            for a_np in (None, age, clamp):
                a_d = None if a_np is None else torch.from_numpy(a_np).cuda()
                for sig in (False, True):
                    ref = oracle_logits(m, feats, a_np, sig)
                    got = eng.lstm_head(fd, a_d, apply_sigmoid=sig)
                    torch.cuda.synchronize()
                    assert got.shape == (S, N)
                    worst = max(worst, assert_logits(
                        got, ref, f"{name} S={S} N={N} sigmoid={sig}"))
                    if a_np is clamp:
                        off = got[:, ::2].cpu()
                        want = 0.5 if sig else 0.0
                        assert (off == want).all()
                        assert (ref[:, ::2] == want).all()
        print(f"[lstm head] {name} N={N}: max |err| = {worst:.3e}")

    @pytest.mark.parametrize("name", HEAD_VARIANTS)
    def test_rows_independent_under_permutation(self, name):
        m = head_model(name)
        eng = engine_for(name, m, key=("head", name))
        for S, N in ((5, 33), (9, 65), (9, 3)):
            feats, age = head_inputs(eng.feat_len, S, N)
            fd = torch.from_numpy(feats).cuda()
            ad = torch.from_numpy(age).cuda()
            base = eng.lstm_head(fd, ad, apply_sigmoid=False).clone()
            perm = torch.from_numpy(
                np.random.default_rng(S + N).permutation(S)).cuda()
            got = eng.lstm_head(fd[perm].contiguous(), ad[perm].contiguous(),
                                apply_sigmoid=False)
            torch.cuda.synchronize()
            assert torch.equal(got, base[perm]), (S, N)
            # ... nor on how many rows there are
            one = eng.lstm_head(fd[S - 1:].contiguous(),
                                ad[S - 1:].contiguous(), apply_sigmoid=False)
            assert torch.equal(one[0], base[S - 1]), (S, N)


# --------------------------------------------------------------------------
# 6. GPU: more windows / sequences / streams than the launchers' grid cap
# --------------------------------------------------------------------------
@pytest.mark.gpu
class TestPastGridCap:
    """Every launcher caps its grid at 8192 blocks; these run the grid-stride
    loops with their reused LDS. The inputs repeat 61 distinct exact items
    (odd: pairs and workgroups never align with the period)."""

    @pytest.mark.parametrize("kernel,sn", [("fp32", GRID_CAP * 4 + 7),
                                           ("staged", GRID_CAP * 4 + 7),
                                           ("tlast", GRID_CAP * 8 + 3)])
    def test_conv(self, kernel, sn):
        _, x, ref = exact_case("MyCNN5")
        eng = engine_for("MyCNN5")
        idx = torch.arange(sn, device="cuda") % PERIOD
        xin = conv_input(kernel, dev(x[:PERIOD])[idx])
        got = eng.conv_features(xin).reshape(sn, -1)
        torch.cuda.synchronize()
        # every repeat of a pattern window is the same bits ...
        first = got[:PERIOD]
        assert torch.equal(got, first[idx])
        # ... and the 61 are the oracle's
        worst = assert_feats(first.cpu(), ref[:PERIOD], f"{kernel} SN={sn}")
        print(f"[grid cap] {kernel} SN={sn}: max |err| = {worst:.3e}")

    def test_score_latest(self, monkeypatch):
        # the split bucket layout keeps the largest allocation at the ring's
        # own size (S * 10 * 128 * 4 bytes, about 335 MB)
        monkeypatch.setenv("TSKD_PACKED_BUCKETS", "0")
        S, G, nproc = GRID_CAP * 8 + 3, 128, 136      # window across the wrap
        m, _, _ = exact_case("MyCNN5")
        eng = engine_for("MyCNN5")
        pattern = exact_windows(10, n=PERIOD, length=G, seed=6)
        se, idx = ring_engine(S, G, pattern)
        se.nproc = nproc
        age61 = stream_ages(PERIOD)
        age = torch.from_numpy(age61[idx]).cuda()
        feats = oracle_features(m, ring_windows(pattern, G, nproc),
                                bf16_path=True).reshape(PERIOD, 1, -1)
        ref = oracle_logits(m, feats, age61, False)
        got = se.score_latest(eng, age, apply_sigmoid=False)
        torch.cuda.synchronize()
        assert got.shape == (S, 1)
        first = got[:PERIOD]
        assert torch.equal(got, first[torch.from_numpy(idx).cuda()])
        worst = assert_logits(first, ref, f"score_latest S={S}")
        print(f"[grid cap] score_latest S={S}: max |err| = {worst:.3e}")

    def test_lstm_head(self):
        S, N = GRID_CAP * 4 + 5, 2
        m = head_model("MyCNN5")
        eng = engine_for("MyCNN5", m, key=("head", "MyCNN5"))
        feats, age = head_inputs(eng.feat_len, PERIOD, N)
        idx = torch.arange(S, device="cuda") % PERIOD
        fd = torch.from_numpy(feats).cuda()[idx].contiguous()
        ad = torch.from_numpy(age).cuda()[idx].contiguous()
        got = eng.lstm_head(fd, ad, apply_sigmoid=False)
        torch.cuda.synchronize()
        first = got[:PERIOD]
        assert torch.equal(got, first[idx])
        worst = assert_logits(first, oracle_logits(m, feats, age, False),
                              f"lstm_head S={S}")
        print(f"[grid cap] lstm_head S={S} N={N}: max |err| = {worst:.3e}")


# --------------------------------------------------------------------------
# 7. GPU: a non-finite value stays in its own window
# --------------------------------------------------------------------------
# Window j + 1 is poisoned at t = 0, 1, 2 in every channel and window j must
# not notice. "pair": every odd window, so j and j + 1 are one wave's pair in
# the pair kernels. "apart": every fourth window, so j and j + 1 belong to
# different waves, and at every second one to different workgroups, in every
# kernel (4 windows per workgroup, 8 in the pair kernels). Many j at once,
# because fmaxf drops a NaN operand: a NaN in window j's last conv1 rows
# changes its features only where the poisoned pool cell held the maximum.
POISONED = {"pair": list(range(1, NWIN, 2)), "apart": list(range(4, NWIN, 4))}
BAD = {"nan": float("nan"), "inf": float("inf")}


def assert_others_unchanged(f1, f0, poisoned, what):
    keep = [i for i in range(f0.shape[0]) if i not in poisoned]
    changed = [i for i in keep if not torch.equal(f1[i], f0[i])]
    assert not changed, (
        f"{what}: a non-finite value at t = 0..2 of the NEXT window changed "
        f"{len(changed)} of {len(keep)} clean windows, first {changed[:8]}")


@pytest.mark.gpu
class TestNonFiniteIsolation:
    @pytest.mark.parametrize("where", sorted(POISONED))
    @pytest.mark.parametrize("bad", sorted(BAD))
    @pytest.mark.parametrize("kernel,name", kernel_cases())
    def test_conv_next_window(self, kernel, name, bad, where):
        _, x, ref = exact_case(name)
        eng = engine_for(name)
        xd = dev(x)
        f0 = run_conv(eng, kernel, conv_input(kernel, xd))
        assert_feats(f0, ref, f"{kernel} {name} clean")
        xp = xd.clone()
        xp[POISONED[where], :, 0:3] = BAD[bad]
        xin = conv_input(kernel, xp)
        assert int((~torch.isfinite(xin.float())).sum()) == \
            3 * xd.shape[1] * len(POISONED[where])
        f1 = run_conv(eng, kernel, xin)
        assert_others_unchanged(f1, f0, POISONED[where],
                                f"{kernel} {name} {bad} {where}")

    @pytest.mark.parametrize("where", sorted(POISONED))
    @pytest.mark.parametrize("bad", sorted(BAD))
    @pytest.mark.parametrize("name", TLAST_VARIANTS)
    def test_score_latest_next_stream(self, name, bad, where):
        eng = engine_for(name)
        S, nproc = NWIN, 200
        pattern = exact_windows(10, n=S, length=RING_G, seed=7)
        se, _ = ring_engine(S, RING_G, pattern)
        se.nproc = nproc
        s0 = se.score_latest(eng, None, apply_sigmoid=False).clone()
        assert torch.isfinite(s0).all()
        # the window's t = 0, 1, 2 in stream s + 1's ring row
        slots = (torch.arange(nproc - 120, nproc - 117) % RING_G).tolist()
        for s in POISONED[where]:
            se.proc[s, :, slots] = BAD[bad]
        s1 = se.score_latest(eng, None, apply_sigmoid=False)
        torch.cuda.synchronize()
        assert_others_unchanged(s1.cpu(), s0.cpu(), POISONED[where],
                                f"score_latest {name} {bad} {where}")

    @pytest.mark.parametrize("name", TLAST_VARIANTS)
    def test_slack_contents_do_not_matter(self, name):
        """Garbage in an alloc_windows buffer's slack reaches no window, the
        last one included: the slack has to be addressable, nothing more."""
        _, x, ref = exact_case(name)
        eng = engine_for(name)
        for sn in (1, 8, 9):
            xin = conv_input("tlast", dev(x)[:sn])
            f0 = run_conv(eng, "tlast", xin)
            assert_feats(f0, ref[:sn], f"tlast {name} SN={sn} clean")
            numel = xin.numel()
            assert xin._tskd_buf.numel() > numel
            for bad in sorted(BAD):
                xin._tskd_buf[numel:] = BAD[bad]
                f1 = run_conv(eng, "tlast", xin)
                assert torch.equal(f1[:sn - 1], f0[:sn - 1]), (name, sn, bad)
                assert torch.equal(f1[sn - 1], f0[sn - 1]), (
                    f"{name} SN={sn}: {bad} in the slack changed the last "
                    f"window")
