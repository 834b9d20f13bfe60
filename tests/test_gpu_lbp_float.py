"""ExtendedLBP, OriginalLBP and LPQ on float32 / float64 images (ofr_lbp_float.hip, lpq_kernel<float|double>):
code images, fused cell counts and the LBPH model behind a preprocessing step, against float64 numpy
restatements of the three formulas.

ExtendedLBP: the elbp_geometry weights, the sequential fp64 sum without zero-weight terms, and the reference's
uint8 centre C = trunc(x).astype(int64) & 255.  OriginalLBP: >= on the values as given.  Both bit-exact.
LPQ codes are signs of G = V^T F; every case first asserts that its own reference has min |G| > 1e-6, as
tests/test_gpu_descriptors.py.  Distances: 1e-10 relative, as tests/test_gpu_hist_metrics.py.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-10
GUARD = 1e-6
KINDS = {"tantriggs-like": (np.float32, -10.0, 10.0), "equalisation-like": (np.float64, 0.0, 255.0)}
SHAPES = [
    (1, 13, 18, (2, 3)),      # non-square, grid remainder
    (1, 18, 13, (2, 2)),      # odd pitch: every load alignment
    (2, 5, 6, (1, 2)),        # smaller than the LPQ window
    (3, 40, 36, (2, 2)),      # 16-bit counts, n = 3
    (1, 9, 70, (1, 4)),       # wider than a wave
    (2, 40, 36, (14, 12)),    # more counters than LDS holds: two bands of cell rows per image
]
DESCS = [("elbp", 1, 8), ("olbp", 0, 8), ("lpq", 1, 8), ("lpq", 2, 8), ("lpq", 3, 8)]
CASES = [(d, s) for s in SHAPES for d in DESCS] + [
    (("elbp", 2, 8), SHAPES[3]),                    # the generic (radius, P) form
    (("elbp", 2, 12), (1, 9, 70, (1, 12))),         # 12 x 4096 counters: one cell row exceeds LDS, global counters
]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    torch.cuda.set_device(0)


def operator(desc):
    from ocvfacerec.facerec.lbp import LPQ, ExtendedLBP, OriginalLBP
    name, radius, P = desc
    return {"elbp": lambda: ExtendedLBP(radius, P), "olbp": OriginalLBP, "lpq": lambda: LPQ(radius)}[name]()


def elbp_ref(X, radius, P):
    from ocvfacerec.facerec.lbp import elbp_geometry
    (oy, ox), (by, bx), offs, wts = elbp_geometry(radius, P)
    X = X.astype(np.float64)
    dy, dx = X.shape[0] - by + 1, X.shape[1] - bx + 1
    C = (np.trunc(X[oy:oy + dy, ox:ox + dx]).astype(np.int64) & 255).astype(np.float64)
    codes = np.zeros((dy, dx), np.int64)
    for i, ((fy, fx, cy, cx), w) in enumerate(zip(offs, wts)):
        N = None
        for (ty, tx), wt in zip(((fy, fx), (fy, cx), (cy, fx), (cy, cx)), w):
            if wt != 0.0:
                term = wt * X[ty:ty + dy, tx:tx + dx]
                N = term if N is None else N + term
        codes |= (N >= C).astype(np.int64) << i
    return codes


def olbp_ref(X):
    X = X.astype(np.float64)
    c = X[1:-1, 1:-1]
    ring = [X[0:-2, 0:-2], X[0:-2, 1:-1], X[0:-2, 2:], X[1:-1, 2:], X[2:, 2:], X[2:, 1:-1], X[2:, :-2], X[1:-1, :-2]]
    return sum((1 << (7 - i)) * (nb >= c) for i, nb in enumerate(ring))


def lpq_ref(X, r, V):
    """-> (codes [H][W] in the reference's order, min |G|)."""
    H, W = X.shape
    w1 = np.exp(-2j * np.pi * np.arange(-r, r + 1) / (2 * r + 1))
    w0, w2 = np.ones(2 * r + 1), np.conj(w1)
    P = np.zeros((H + 2 * r, W + 2 * r))
    P[r:r + H, r:r + W] = X
    F = []
    for a, b in ((w0, w1), (w1, w0), (w1, w1), (w1, w2)):   # Q(y, x) = sum a(u) b(v) X(y - u, x - v)
        Q = sum(a[i] * b[j] * P[2 * r - i:2 * r - i + H, 2 * r - j:2 * r - j + W]
                for i in range(2 * r + 1) for j in range(2 * r + 1))
        F += [Q.real.flatten("F"), Q.imag.flatten("F")]
    G = V.T @ np.array(F)
    return ((G >= 0) * (1 << np.arange(8))[:, None]).sum(0).reshape(H, W), np.abs(G).min()


def ref_codes(desc, x):
    name, radius, P = desc
    if name == "elbp":
        return elbp_ref(x, radius, P)
    if name == "olbp":
        return olbp_ref(x)
    codes, gmin = lpq_ref(x, radius, operator(desc).basis())
    assert gmin > GUARD
    return codes


@functools.lru_cache(maxsize=None)
def case(desc, kind, n, H, W):
    """Images and their reference code images, computed once per shape."""
    dt, lo, hi = KINDS[kind]
    X = np.random.default_rng(0).uniform(lo, hi, (n, H, W)).astype(dt)
    return X, [ref_codes(desc, x) for x in X]


def cell_counts(codes, grid, nbins=256):
    """feature.py:286-302 as integers: [cells][nbins], and the cell's pixel count."""
    py, px = codes.shape[0] // grid[0], codes.shape[1] // grid[1]
    out = [np.bincount(codes[r * py:(r + 1) * py, c * px:(c + 1) * px].ravel(), minlength=nbins)
           for r in range(grid[0]) for c in range(grid[1])]
    return np.array(out), py * px


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("desc,shape", CASES)
def test_codes_and_counts(desc, shape, kind):
    from opencv_facerecognizer_amd import _device
    from ocvfacerec.facerec.feature import SpatialHistogram
    n, H, W, grid = shape
    X, refs = case(desc, kind, n, H, W)
    op = operator(desc)
    for x, ref in zip(X, refs):
        assert np.array_equal(op(x), ref)
    sh = SpatialHistogram(op, grid)
    want = [cell_counts(ref, grid, 1 << desc[2]) for ref in refs]
    for src in (list(X), torch.from_numpy(X).cuda()):   # a host list and a device tensor
        counts, cell, cb = sh.counts_device(src)
        assert cell == want[0][1] and cb == (1 if cell <= 255 else 2)
        assert np.array_equal(_device.counts_numpy(counts, cb).astype(np.int64), np.array([w for w, _ in want]))
    assert np.array_equal(sh.extract(X[-1]), (want[-1][0] / float(cell)).reshape(-1))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_integer_valued_floats_match_the_byte_kernels(dtype):
    from opencv_facerecognizer_amd import _device
    from ocvfacerec.facerec.lbp import elbp_geometry
    Xb = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (2, 18, 13)).astype(np.uint8)).cuda()
    Xf = Xb.to(dtype)
    assert torch.equal(_device.elbp_codes(Xf, elbp_geometry(1, 8)), _device.elbp_codes(Xb, elbp_geometry(1, 8)))
    assert torch.equal(_device.olbp_codes(Xf), _device.olbp_codes(Xb))


MODELS = [(p, d, "ChiSquareDistance") for p in ("TanTriggsPreprocessing", "HistogramEqualization")
          for d in (("elbp", 1, 8), ("lpq", 1, 8))] + [("TanTriggsPreprocessing", ("elbp", 1, 8), "HistogramIntersection")]


@pytest.mark.parametrize("pre,desc,metric", MODELS)
def test_lbph_model_behind_preprocessing(pre, desc, metric):
    import ocvfacerec.facerec.distance as D
    import ocvfacerec.facerec.preprocessing as PP
    from ocvfacerec.facerec.classifier import NearestNeighbor
    from ocvfacerec.facerec.feature import SpatialHistogram
    from ocvfacerec.facerec.model import PredictableModel
    from ocvfacerec.facerec.operators import ChainOperator
    from opencv_facerecognizer_amd._device import Chi2Gallery
    r = np.random.default_rng(7)
    X = r.integers(0, 256, (12, 16, 16)).astype(np.uint8)    # 3 identities x 4 faces
    y = np.arange(12) % 3
    Q = np.clip(X.astype(np.int64) + r.integers(-2, 3, X.shape), 0, 255).astype(np.uint8)
    grid = (2, 2)
    step = getattr(PP, pre)()
    model = PredictableModel(ChainOperator(step, SpatialHistogram(operator(desc), grid)),
                             NearestNeighbor(getattr(D, metric)(), k=1))
    model.compute(list(X), y)      # raises without the float kernels
    cell = 49 if desc[0] == "elbp" else 64   # 14 x 14 / 16 x 16 codes in 2 x 2 cells
    g = model.classifier.__dict__["_dev"][2]   # adopted from the feature's device counts, not rebuilt
    assert model._lbph() and isinstance(g, Chi2Gallery) and g.count_bytes == 1 and g.denom == float(cell)
    for x, f in zip(X, model.classifier.X):
        want, c = cell_counts(ref_codes(desc, step.extract(x)), grid)
        assert c == cell and np.array_equal(np.asarray(f), (want / float(cell)).reshape(-1))
    single = [model.predict(q) for q in Q]     # the one-face route: extract, then classify
    for batch in (list(Q), torch.from_numpy(Q).cuda()):
        preds = model.predict_batch(batch)
        assert [p[0] for p in preds] == [s[0] for s in single]
        np.testing.assert_allclose([p[1]["distances"][0] for p in preds], [s[1]["distances"][0] for s in single],
                                   rtol=RTOL, atol=0)


def test_other_device_dtypes_are_a_type_error():
    from ocvfacerec.facerec.feature import SpatialHistogram
    with pytest.raises(TypeError):
        SpatialHistogram().counts_batch(torch.zeros((1, 16, 16), dtype=torch.int32, device="cuda"))
