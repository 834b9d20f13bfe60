"""Illumination-normalisation throughput: ofr_tantriggs_f32 and ofr_histeq_f64 on 4,096 resident faces of
128x128 (uint8 in HBM, as ingest.faces leaves them).

Timed with HIP events around `reps` back-to-back launches on the current stream after a warm-up; the
figure is the median of `samples` such windows, with the min..max spread beside it.  Roofline against HBM
with the algorithmic bytes: 1 byte in + 4 out per pixel for Tan-Triggs, 1 + 8 for the equalisation.  The
host baseline is the reference's own numpy/scipy code (preprocessing.py:98-105, 73-77, with density=True)
on a sample of the same faces, 1 thread, scaled to the batch.  Prints one JSON line.

    python tools/bench_preproc.py [--faces 4096] [--size 128]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opencv_facerecognizer_amd import _device, _lib  # noqa: E402

PEAK_HBM = 8.0e12
TT = dict(alpha=0.1, tau=10.0, gamma=0.2, sigma0=1.0, sigma1=2.0)


def windows(fn, reps, samples):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def tantriggs_host(x):
    from scipy import ndimage
    X = np.power(np.array(x, dtype=np.float32), TT["gamma"])
    X = np.asarray(ndimage.gaussian_filter(X, TT["sigma1"]) - ndimage.gaussian_filter(X, TT["sigma0"]))
    X = X / np.power(np.mean(np.power(np.abs(X), TT["alpha"])), 1.0 / TT["alpha"])
    X = X / np.power(np.mean(np.power(np.minimum(np.abs(X), TT["tau"]), TT["alpha"])), 1.0 / TT["alpha"])
    return TT["tau"] * np.tanh(X / TT["tau"])


def histeq_host(x, num_bins=256):
    h, b = np.histogram(x.flatten(), num_bins, density=True)
    cdf = h.cumsum()
    cdf = 255 * cdf / cdf[-1]
    return np.interp(x.flatten(), b[:-1], cdf).reshape(x.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=4096)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--samples", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_preproc needs the GPU")
    n, s = a.faces, a.size
    X = np.random.Generator(np.random.PCG64(20261126)).integers(0, 256, (n, s, s), dtype=np.uint8)
    Xd = torch.from_numpy(X).to(_lib.device())
    res = {"metric": "faces/s, illumination normalisation of resident uint8 faces", "data": "synthetic",
           "faces": n, "size": [s, s], "reps": a.reps, "samples": a.samples}
    m = 32
    for name, fn, host, bpp in (("tantriggs", lambda: _device.tantriggs(Xd, **TT), tantriggs_host, 5),
                                ("histeq", lambda: _device.histeq(Xd, 256), histeq_host, 9)):
        med, lo, hi = windows(fn, a.reps, a.samples)
        alg = float(n) * s * s * bpp
        t0 = time.perf_counter()
        ref = [host(X[j]) for j in range(m)]
        t_host = (time.perf_counter() - t0) / m
        err = float(np.abs(fn()[:m].cpu().numpy() - np.stack(ref)).max())
        res[name] = {"ms": med, "ms_min": lo, "ms_max": hi, "faces_per_s": n / (med * 1e-3),
                     "roofline": {"bound": "hbm", "algorithmic_bytes": alg, "achieved_gbs": alg / (med * 1e-3) / 1e9,
                                  "peak_gbs": PEAK_HBM / 1e9, "frac": alg / (med * 1e-3) / PEAK_HBM},
                     "max_abs_diff_vs_host_sample": err,
                     "cpu_baseline": {"kind": "reference numpy/scipy", "cores": 1, "faces_per_s": 1.0 / t_host,
                                      "batch_ms": t_host * n * 1e3, "sample": f"{m} faces"}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
