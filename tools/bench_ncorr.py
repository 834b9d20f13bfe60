"""NormalizedCorrelation 1-NN search at the BASELINE.json configs[3] shape: ExtendedLBP(1,8) +
SpatialHistogram 8x8 uint8 counts (16,384 bins) of 65,536 gallery faces, B = 4,096 queries.  Prints one
JSON line.

    python tools/bench_ncorr.py [--gallery 65536] [--batch 4096] [--reps 7]

Faces as tools/bench_lbp_chi2.py (synthetic, generated on the device).  Timed with HIP events after a
warm-up call, median of --reps single calls, NormalizedCorrelation and ChiSquare alternating on the same
gallery bytes:
  ncorr_knn_ms     one ofr_ncorr_knn call: row statistics of both operands, the int8-MFMA coarse pass and the
                   fp64 re-rank with its certificate (the coarse kernel alone is not split out: that takes a
                   kernel trace);
  ncorr_search_ms  Chi2Gallery.search: the same plus the exact pass for uncertified queries;
  chi2_search_ms   the ChiSquare search (ofr_chi2_knn and its fallback) on the same counts.
int8_frac: 2 B N nbins int8 operations over the ofr_ncorr_knn time, against the 5 POPS dense int8 peak --
an end-to-end rate of that call, a lower bound of the coarse kernel's own share.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opencv_facerecognizer_amd import _lib  # noqa: E402
from opencv_facerecognizer_amd._device import Chi2Gallery  # noqa: E402
from opencv_facerecognizer_amd.facerec.feature import SpatialHistogram  # noqa: E402
from opencv_facerecognizer_amd.facerec.lbp import ExtendedLBP  # noqa: E402
from opencv_facerecognizer_amd.synthetic import SEED, IdentityBank  # noqa: E402

PEAK_I8_MFMA = 5.0e15   # dense int8 MFMA, MI355X


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--per-id", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    device = _lib.device()
    N, B, H = args.gallery, args.batch, 128
    n_ids = (N + args.per_id - 1) // args.per_id
    bank = IdentityBank(n_ids, H, H, device=device)
    G_img = bank.images(torch.arange(N, device=device) // args.per_id, seed=SEED + 11).reshape(N, H, H)
    gq = torch.Generator(device=device)
    gq.manual_seed(SEED + 12)
    ids_q = torch.randint(0, n_ids, (B,), generator=gq, device=device)
    Q_img = bank.images(ids_q, seed=SEED + 13).reshape(B, H, H)
    sh = SpatialHistogram(ExtendedLBP(1, 8), (8, 8))
    gc, cell, _ = sh.counts_device(G_img)
    qc, _, _ = sh.counts_device(Q_img)
    del G_img, Q_img
    nb = gc.shape[1] * gc.shape[2]
    G = gc.reshape(N, nb)
    Qc = qc.reshape(B, nb).contiguous()
    ncc = Chi2Gallery(G, dtype=_lib.DT_U8, denom=float(cell), nbins=nb, metric=_lib.METRIC_NCORR)
    chi = Chi2Gallery(G, dtype=_lib.DT_U8, denom=float(cell), nbins=nb)

    out_d = torch.empty((B, 1), dtype=torch.float64, device=device)
    out_i = torch.empty((B, 1), dtype=torch.int64, device=device)
    cert = torch.empty(B, dtype=torch.int32, device=device)
    ws = ncc.ws.get(_lib.load().ofr_ncorr_workspace_bytes(B, N, 1), device)

    def knn():
        _lib.call("ofr_ncorr_knn", _lib.stream(), _lib.DT_U8, _lib.ptr(Qc), B, nb, _lib.ptr(ncc.G), N, ncc.G.shape[1],
                  nb, 1, 0, _lib.ptr(out_d), _lib.ptr(out_i), _lib.ptr(ws), ws.numel(), _lib.ptr(cert))

    runs = {"ncorr_knn_ms": knn, "ncorr_search_ms": lambda: ncc.search(Qc, 1), "chi2_search_ms": lambda: chi.search(Qc, 1)}
    for fn in runs.values():   # warm-up: code objects, workspaces
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(args.reps):
        for name, fn in runs.items():
            times[name].append(once(fn)[0])
    _, (dd, ii) = once(runs["ncorr_search_ms"])
    ops = 2.0 * B * N * nb
    med = {name: statistics.median(t) for name, t in times.items()}
    out = {"metric": "NormalizedCorrelation 1-NN over LBPH uint8 counts (configs[3] shape)",
           "config": {"gallery": N, "batch": B, "bins": nb, "k": 1, "reps": args.reps}, "data": "synthetic",
           **med, "spread_ms": {name: [min(t), max(t)] for name, t in times.items()},
           "int8_ops": ops, "int8_tops_of_knn_call": ops / (med["ncorr_knn_ms"] * 1e-3) / 1e12,
           "int8_frac_of_knn_call": ops / (med["ncorr_knn_ms"] * 1e-3) / PEAK_I8_MFMA,
           "ncorr_uncertified": list(ncc.last_fallbacks), "chi2_uncertified_after_each_pass": list(chi.last_fallbacks),
           "top1_identity_acc": float(((ii[:, 0] // args.per_id) == ids_q).double().mean().item())}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
