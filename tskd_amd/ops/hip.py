"""ctypes bindings for the three HIP kernel libraries.

One signature table, one loader, and the small helpers every launch needs.
To expose a new entry point, add it to the ``extern "C"`` block of its .hip
file and one line to ``SIGNATURES``; tests/test_hip_bindings.py parses the
prototypes and fails until both agree. Every entry point returns ``int``
(0, a hipError, or a launcher's own negative code).
"""

from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional

import torch

from tskd_amd.ops import build as _build

MYCNN, PREPROC, TRAIN = "_tskd_mycnn", "_tskd_preprocess", "_tskd_train"

P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
U64 = ctypes.c_ulonglong

SIGNATURES = {
    MYCNN: {
        "tskd_serve_tail_fwd": [P, I, I, I, L, P, I, P, P, P, P, F, I, I, P],
        "tskd_serve_tail_occlude_fwd": [P, I, I, I, L, P, I, P, I, P, P, P, F,
                                        I, I, P],
        "tskd_serve_tail_history_fwd": [P, I, I, I, L, P, I, P, I, I, I, P, P,
                                        P, F, I, I, P],
        "tskd_conv_fwd": [P, I, I, P, P, P, I, I, P],
        "tskd_lstm_head_fwd": [P, P, P, P, I, I, F, I, I, P],
        "tskd_debug_mfma16x16x32": [P, P, P, P],
        "tskd_pack_size": [I],
        "tskd_feat_len": [I],
    },
    PREPROC: {
        "tskd_preproc_ingest_dense": [P, I, P, P, P, I, I, I, I, I, I, L, P,
                                      I, P],
        "tskd_preproc_ingest_dense_gated": [P, I, P, P, P, I, I, I, I, I, I,
                                            L, P, I, P, P, P],
        "tskd_preproc_ingest_events": [P, P, P, P, P, P, I, I, L, L, I, P],
        "tskd_preproc_ingest_events_gated": [P, P, P, P, P, P, I, I, L, L, I,
                                             P, P, P],
        "tskd_preproc_clear_buckets": [P, P, I, I, I, L, I, I, P],
        "tskd_preproc_reset_streams": [P, I, P, P, P, P, I, I, I, I, P],
        "tskd_preproc_snapshot_streams": [P, I, P, P, P, P, I, I, I, I, L, I,
                                          I, P, P],
        "tskd_preproc_restore_streams": [P, I, P, P, P, P, I, I, I, I, L, I,
                                         I, P, P],
        "tskd_preproc_window_coverage": [P, I, P, I, I, I, I, L, I, I, L, P,
                                         P],
        "tskd_preproc_window_fill": [P, P, P, P, I, I, I, L, I, I, P, I, P],
        "tskd_preproc_advance_state": [P, I, I, P],
        "tskd_preproc_window_gather": [P, P, I, I, I, I, I, I, I, I, L, P, I,
                                       P],
        "tskd_preproc_window_znorm": [P, I, L, I, F, P],
    },
    TRAIN: {
        "tskd_train_batch_accuracy": [P, P, P, L, P],
        "tskd_train_conv_fwd": [P, P, P, P, I, F, F, U64, I, P],
        "tskd_train_lstm_fwd": [P, P, P, P, P, I, I, F, I, P],
        "tskd_train_loss": [P, P, P, P, P, L, F, F, P],
        "tskd_train_lstm_bwd": [P, P, P, P, P, P, I, I, I, P],
        "tskd_train_conv_bwd": [P, P, P, P, P, I, I, P],
        "tskd_train_adam": [P, P, P, P, L, F, F, F, F, I, P],
        "tskd_train_stash_sizes": [I, P, P],
    },
}

# exported by a .hip file but deliberately not bound
UNBOUND = {"tskd_conv_ksteps"}

_libs: Dict[str, ctypes.CDLL] = {}


def load(name: str) -> ctypes.CDLL:
    """The named library with every table entry typed; cached. Built first
    only when the .so is missing (a stale one is loaded as it is)."""
    lib = _libs.get(name)
    if lib is None:
        path = _build.lib_path(name)
        if not os.path.exists(path):
            try:
                _build.build(name)
            except Exception as e:
                raise RuntimeError(f"hipcc build failed: {e}") from e
        lib = _libs[name] = open_lib(name, path)
    return lib


def use_lib(name: str, lib: ctypes.CDLL) -> None:
    """Make ``lib`` (from :func:`open_lib`) what :func:`load` returns for
    ``name`` from now on: scripts/ab_bench.py times two builds of a library
    against each other by swapping them per round."""
    _libs[name] = lib


def open_lib(name: str, path: str) -> ctypes.CDLL:
    """The build of library ``name`` at ``path`` with every table entry
    typed; not cached (see :func:`use_lib`)."""
    lib = ctypes.CDLL(path)
    for fn, argtypes in SIGNATURES[name].items():
        entry = getattr(lib, fn)
        entry.restype = I
        entry.argtypes = argtypes
    return lib


def ptr(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    """Device pointer of ``t``; None is the null pointer."""
    return P(0 if t is None else t.data_ptr())


def stream_ptr() -> ctypes.c_void_p:
    """The current torch stream as a hipStream_t."""
    return P(torch.cuda.current_stream().cuda_stream)


def check(rc: int, what: str) -> None:
    """Raise if entry point ``what`` returned a nonzero code."""
    if rc != 0:
        raise RuntimeError(f"{what} failed: code {rc}")
