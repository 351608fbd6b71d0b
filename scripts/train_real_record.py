#!/usr/bin/env python3
"""End-to-end training on the committed REAL p000194 numerics record
(VERDICT r1 #5): WFDB decode (C++ reader) -> reference ETL (5-s resample,
3-min rolling mean, interpolate) -> label windows -> class rebalance ->
BOTH trainers (torch-eager reference recipe AND the HIP kernel trainer on
GPU) -> legacy-pickle checkpoint loadable exactly the way the reference
serving loads it (predictStream.py:36-38: `from models import MyCNN` into
__main__, `torch.load(path)`) -> evaluation report with sklearn baselines.

Labels: p000194 has NO cardiac-arrest annotation in the committed cohort
table (data/patients_waveform.csv lists 44 other records whose waveforms
were never committed), so the CA time here is SYNTHETIC: the record end is
treated as the arrest time, making the last 2 h positive — the reference's
exact labeling geometry (explore_torch.ipynb cell 2) on real vitals. The
resulting AUC is a machinery check, not a clinical claim; the reference's
own ~0.66 AUC used 44 records we cannot download (no network).

Channel-name parity note: the record names NBP channels "NBPSys" etc.
while config.cfg says "NBP Sys" — the reference ETL zero-fills configured
channels missing from the record, so those columns are zero there AND here.

Usage: python scripts/train_real_record.py [--epochs 250] [--out-dir artifacts]
"""
from __future__ import annotations

import argparse
import datetime
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(
    REPO, "data/waveform/physionet.org/files/mimic3wdb-matched/1.0/p00/"
    "p000194/p000194-2112-05-23-14-34n")
AGE_CSV = os.path.join(REPO, "data/patients_age.csv")


def age_from_cohort(subject_id: int, record_date: datetime.date) -> float:
    """Age at record time from the committed cohort table (reference
    db_exploration.ipynb join semantics: DOB -> age)."""
    with open(AGE_CSV) as f:
        next(f)
        for ln in f:
            sid, dob = ln.strip().split(",")[:2]
            if int(sid) == subject_id:
                d = datetime.date.fromisoformat(dob)
                return (record_date - d).days / 365.25
    return float("nan")


def etl(epochs_note=None, valid_range_specs=None):
    from tskd_amd.config import get_global_config, resolve_valid_ranges
    from tskd_amd.io import rdrecord
    from tskd_amd.train.data import (clamp_age, label_windows,
                                     record_to_training_frame)
    cfg = get_global_config()
    rec = rdrecord(RECORD)
    dur_s = rec.sig_len / rec.fs
    df = record_to_training_frame(
        rec.p_signal, rec.fs, rec.sig_name, cfg.channel_names,
        valid_range=resolve_valid_ranges(cfg, valid_range_specs))
    # synthetic CA time at record end: last 2 h positive (see module doc)
    x, y = label_windows(df, ca_time_s=dur_s,
                         window_size=cfg.window_size,
                         overlap_pct=cfg.record_overlap)
    x = np.nan_to_num(x, nan=0.0).astype(np.float32)
    age = clamp_age(age_from_cohort(194, datetime.date(2112, 5, 23)))
    ages = np.full(len(y), age, dtype=np.float32)
    return x, ages, y.astype(np.float32), {
        "record": os.path.basename(RECORD), "sig_names": rec.sig_name,
        "fs_hz": rec.fs, "sig_len": rec.sig_len,
        "duration_h": round(dur_s / 3600, 2),
        "grid_points": len(df), "n_windows": int(len(y)),
        "n_pos": int(y.sum()), "age_years": round(age, 1),
    }


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=250)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "artifacts"))
    ap.add_argument("--hip", action="store_true", default=None,
                    help="also run the HIP kernel trainer (needs GPU; "
                         "auto when CUDA is available)")
    ap.add_argument("--valid-range", action="append", default=None,
                    metavar="SPEC",
                    help="train on what a gated daemon serves (repeatable): "
                         "NAME=LO:HI or the preset 'numerics', as serve "
                         "--valid-range; out-of-range samples become "
                         "missing before the 5 s resample")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    use_hip = args.hip if args.hip is not None else torch.cuda.is_available()

    x, ages, y, meta = etl(valid_range_specs=args.valid_range)
    print(f"[etl] {json.dumps(meta)}", flush=True)
    # stratified chronological-ish split (single record): every 3rd window
    # to validation, like the reference's per-record SPLIT but in-record
    idx = np.arange(len(y))
    val_m = (idx % 3) == 2
    from tskd_amd.train.data import random_oversample, random_undersample
    xt, at, yt = random_undersample(x[~val_m], ages[~val_m], y[~val_m],
                                    strategy=0.3, seed=0)
    xv, av, yv = random_oversample(x[val_m], ages[val_m], y[val_m], seed=0)
    print(f"[split] train {len(yt)} (pos {int(yt.sum())}), "
          f"val {len(yv)} (pos {int(yv.sum())})", flush=True)

    # ---- trainer 1: torch-eager reference recipe ----------------------
    from tskd_amd.train.trainer import fit
    ckpt = os.path.join(args.out_dir, "MyCNN5_p000194.pth")
    model, hist = fit(xt, at, yt, xv, av, yv, variant="MyCNN5",
                      epochs=args.epochs, batch_size=16, lr=1e-5,
                      checkpoint_path=ckpt, print_freq=10_000, seed=0)
    print(f"[fit] best val loss {hist['best_val_loss']:.4f} "
          f"after {args.epochs} epochs", flush=True)

    # ---- checkpoint round-trip through the REFERENCE loading path -----
    # predictStream.py:36-38 does `from models import MyCNN` (into the
    # __main__ namespace) then torch.load(MODELPATH). Emulate exactly.
    import __main__
    from tskd_amd.models.mycnn import MyCNN
    __main__.MyCNN = MyCNN
    loaded = torch.load(ckpt, weights_only=False)
    loaded.eval()
    with torch.no_grad():
        xa = torch.from_numpy(x[:32]).float()
        aa = torch.from_numpy(ages[:32]).float()
        ref_out = loaded(xa, aa)
        our_out = model(xa, aa)
    rt_err = float((ref_out - our_out).abs().max())
    assert rt_err < 1e-6, f"round-trip mismatch {rt_err}"
    print(f"[ckpt] legacy-pickle round-trip via __main__.MyCNN ok "
          f"(max err {rt_err:.1e}); file {ckpt} "
          f"({os.path.getsize(ckpt)} B)", flush=True)

    # ---- evaluation report -------------------------------------------
    from tskd_amd.train.report import (classification_metrics,
                                      score_model, sklearn_baselines)
    prob_val = score_model(model, xv, av)
    m = classification_metrics(yv, prob_val)
    base = sklearn_baselines(xt.reshape(len(xt), -1).copy(), yt,
                             xv.reshape(len(xv), -1).copy(), yv)
    report = {"etl": meta, "history_tail": {
        "train_loss": hist["train_loss"][-1],
        "val_loss": hist["val_loss"][-1],
        "best_val_loss": hist["best_val_loss"]},
        "val_metrics": {k: v for k, v in m.items() if k != "report"},
        "sklearn_baselines": base,
        "checkpoint": os.path.relpath(ckpt, REPO),
        "roundtrip_max_err": rt_err,
        "label_note": "synthetic CA time at record end (no committed "
                      "annotation for p000194); machinery check only"}

    # ---- trainer 2: HIP kernel trainer (GPU) --------------------------
    if use_hip:
        from tskd_amd.train.hip_trainer import MyCNNHipTrainer
        B = 16
        n = (len(yt) // B) * B
        xs = torch.from_numpy(xt[:n]).reshape(-1, B, 10, 120).cuda()
        as_ = torch.from_numpy(at[:n]).reshape(-1, B).cuda()
        ys = torch.from_numpy(yt[:n]).reshape(-1, B).cuda()
        pos_w = float((yt == 0).sum() / max(yt.sum(), 1))
        from tskd_amd.models import build_model
        torch.manual_seed(0)
        tr = MyCNNHipTrainer(build_model("MyCNN5"), device="cuda",
                             lr=1e-5, pos_weight=pos_w)
        # mini-batch parity with the torch trainer: one optimizer step per
        # 1-sequence chunk (same number of gradient steps per epoch)
        losses = []
        for ep in range(args.epochs):
            ep_loss = 0.0
            for ci in range(xs.shape[0]):
                ep_loss += tr.step(xs[ci:ci + 1], as_[ci:ci + 1],
                                   ys[ci:ci + 1])
            losses.append(ep_loss / xs.shape[0])
        hip_model = tr.export_model().cpu().eval()
        hip_ckpt = os.path.join(args.out_dir, "MyCNN5_p000194_hip.pth")
        from tskd_amd.models import save_checkpoint
        save_checkpoint(hip_model, hip_ckpt)
        prob_hip = score_model(hip_model, xv, av)
        mh = classification_metrics(yv, prob_hip)
        report["hip_trainer"] = {
            "loss_first": losses[0], "loss_last": losses[-1],
            "val_metrics": {k: v for k, v in mh.items() if k != "report"},
            "checkpoint": os.path.relpath(hip_ckpt, REPO)}
        print(f"[hip] loss {losses[0]:.4f} -> {losses[-1]:.4f}, "
              f"val AUC {mh['roc_auc']:.3f}", flush=True)

    out_json = os.path.join(args.out_dir, "train_real_record.json")
    with open(out_json, "w") as f:
        json.dump(report, f, indent=1)
    print(f"[report] {json.dumps(report['val_metrics'])}")
    print(f"[report] written {out_json}", flush=True)


if __name__ == "__main__":
    main()
