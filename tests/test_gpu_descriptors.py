"""OriginalLBP and LPQ (reference lbp.py:55-72, 211-318) on the GPU: code images, fused cell counts and
the LBPH model, against a float64 numpy restatement of the formulas (shift-and-add over the window).

LPQ codes are signs of G = V^T F; the comparison is exact, so every case first asserts that its own
reference has min |G| > 1e-6 (four orders above the fp64 error of sums of <= 289 terms <= 255, far below
what random images give).  Distances: 1e-10 relative, as tests/test_gpu_hist_metrics.py.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-10
GUARD = 1e-6
# descriptor, radius, n, H, W, grid.  LPQ strips are <= 32 image rows and a wave spans 64 pixels of a row;
# OriginalLBP threads make 4 codes each and a workgroup owns a band of cell rows (64 KiB of counters).
CASES = [
    ("lpq", 3, 1, 13, 18, (2, 3)),      # non-square, grid with a remainder
    ("lpq", 1, 1, 18, 13, (2, 2)),      # the other way round, r = 1
    ("lpq", 3, 2, 5, 6, (1, 2)),        # smaller than the window: halos pass both edges
    ("lpq", 3, 3, 40, 36, (2, 2)),      # two strips (counters meet in global memory), 16-bit counts, n = 3
    ("lpq", 2, 1, 9, 70, (1, 4)),       # wider than one wave, bytewise staging
    ("lpq", 1, 2, 40, 36, (14, 12)),    # 168 cells: more counters than LDS holds
    ("olbp", 0, 1, 13, 18, (2, 3)),
    ("olbp", 0, 3, 18, 13, (2, 2)),     # odd image stride: every dword alignment
    ("olbp", 0, 1, 40, 36, (2, 2)),     # 16-bit counts
    ("olbp", 0, 2, 40, 36, (9, 9)),     # two bands of cell rows
]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    torch.cuda.set_device(0)


def operator(desc, radius):
    from ocvfacerec.facerec.lbp import LPQ, OriginalLBP
    return LPQ(radius) if desc == "lpq" else OriginalLBP()


def lpq_taps(r):
    u = np.arange(-r, r + 1)
    w1 = np.exp(-2j * np.pi * u / (2 * r + 1))
    return np.ones(2 * r + 1), w1, np.conj(w1)


def lpq_D(r):
    """lbp.py:244-275: covariance of the eight responses under the rho = 0.95 pixel model."""
    n = 2 * r + 1
    w0, w1, w2 = lpq_taps(r)
    qs = [np.outer(a, b) for a, b in ((w0, w1), (w1, w0), (w1, w1), (w1, w2))]
    M = np.array([part(q).flatten("F") for q in qs for part in (np.real, np.imag)])
    pts = np.stack([np.arange(n * n) % n, np.arange(n * n) // n], 1).astype(float)
    C = 0.95 ** np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    return M @ C @ M.T


def lpq_ref(X, r, V):
    """-> (codes [H][W] in the reference's order, min |G|)."""
    H, W = X.shape
    w0, w1, w2 = lpq_taps(r)
    P = np.zeros((H + 2 * r, W + 2 * r))
    P[r:r + H, r:r + W] = X
    F = []
    for a, b in ((w0, w1), (w1, w0), (w1, w1), (w1, w2)):   # Q(y, x) = sum a(u) b(v) X(y - u, x - v)
        Q = sum(a[i] * b[j] * P[2 * r - i:2 * r - i + H, 2 * r - j:2 * r - j + W]
                for i in range(2 * r + 1) for j in range(2 * r + 1))
        F += [Q.real.flatten("F"), Q.imag.flatten("F")]
    G = V.T @ np.array(F)
    return ((G >= 0) * (1 << np.arange(8))[:, None]).sum(0).reshape(H, W), np.abs(G).min()


def olbp_ref(X):
    X = X.astype(np.int64)
    c = X[1:-1, 1:-1]
    ring = [X[0:-2, 0:-2], X[0:-2, 1:-1], X[0:-2, 2:], X[1:-1, 2:], X[2:, 2:], X[2:, 1:-1], X[2:, :-2], X[1:-1, :-2]]
    return sum((1 << (7 - i)) * (nb >= c) for i, nb in enumerate(ring))


@functools.lru_cache(maxsize=None)
def case(desc, radius, n, H, W):
    """Images and their reference code images, computed once per shape."""
    X = np.random.default_rng(0).integers(0, 256, (n, H, W)).astype(np.uint8)
    if desc == "olbp":
        return X, [olbp_ref(x) for x in X]
    V = operator(desc, radius).basis()
    refs = [lpq_ref(x, radius, V) for x in X]
    assert min(g for _, g in refs) > GUARD
    return X, [c for c, _ in refs]


def cell_counts(codes, grid):
    """feature.py:286-302 as integers: [cells][256], and the cell's pixel count."""
    py, px = codes.shape[0] // grid[0], codes.shape[1] // grid[1]
    out = [np.histogram(codes[r * py:(r + 1) * py, c * px:(c + 1) * px], bins=256, range=(0, 256))[0]
           for r in range(grid[0]) for c in range(grid[1])]
    return np.array(out), py * px


@pytest.mark.parametrize("radius", [1, 2, 3, 8])
def test_lpq_basis_diagonalises_D(radius):
    from ocvfacerec.facerec.lbp import LPQ
    V, D = LPQ(radius).basis(), lpq_D(radius)
    T = V @ D @ V.T
    assert np.abs(T - np.diag(np.diag(T))).max() <= 1e-9 * np.linalg.svd(D, compute_uv=False)[0]
    assert LPQ(radius).basis() is V   # cached per radius


@pytest.mark.parametrize("desc,radius,n,H,W,grid", CASES)
def test_codes_and_counts(desc, radius, n, H, W, grid):
    from opencv_facerecognizer_amd import _device
    from ocvfacerec.facerec.feature import SpatialHistogram
    X, refs = case(desc, radius, n, H, W)
    op = operator(desc, radius)
    for x, ref in zip(X, refs):
        assert np.array_equal(op(x), ref)
    sh = SpatialHistogram(op, grid)
    counts, cell, cb = sh.counts_device(X)
    got = _device.counts_numpy(counts, cb).astype(np.int64)
    want = [cell_counts(ref, grid) for ref in refs]
    assert cell == want[0][1] and cb == (1 if cell <= 255 else 2)
    assert np.array_equal(got, np.array([w for w, _ in want]))
    assert np.array_equal(sh.extract(X[-1]), (want[-1][0] / float(cell)).reshape(-1))


@pytest.mark.parametrize("desc,metric", [("lpq", "ChiSquareDistance"), ("olbp", "HistogramIntersection")])
def test_lbph_model(desc, metric):
    import ocvfacerec.facerec.distance as D
    from ocvfacerec.facerec.classifier import NearestNeighbor
    from ocvfacerec.facerec.feature import SpatialHistogram
    from ocvfacerec.facerec.model import PredictableModel
    from opencv_facerecognizer_amd._device import Chi2Gallery
    r = np.random.default_rng(7)
    X = r.integers(0, 256, (12, 24, 24)).astype(np.uint8)
    y = np.arange(12) % 4
    Q = np.clip(X.astype(np.int64) + r.integers(-2, 3, X.shape), 0, 255).astype(np.uint8)
    op = operator(desc, 3)
    model = PredictableModel(SpatialHistogram(op), NearestNeighbor(getattr(D, metric)(), k=1))
    model.compute(list(X), y)
    g = model.classifier.__dict__["_dev"][2]   # adopted from the feature's device counts, not rebuilt
    assert model._lbph() and isinstance(g, Chi2Gallery) and g.count_bytes == 1
    assert g.denom == (9.0 if desc == "lpq" else 4.0)   # 24x24 / 22x22 codes in 8x8 cells
    preds = model.predict_batch(list(Q))

    def hists(imgs):
        if desc == "lpq":
            refs = [lpq_ref(x, 3, op.basis()) for x in imgs]
            assert min(g for _, g in refs) > GUARD
            codes = [c for c, _ in refs]
        else:
            codes = [olbp_ref(x) for x in imgs]
        return np.array([cell_counts(c, (8, 8))[0].reshape(-1) / float(cell_counts(c, (8, 8))[1]) for c in codes])

    p, q = hists(Q)[:, None, :], hists(X)[None, :, :]
    dist = ((p - q) ** 2 / (p + q + np.finfo("float").eps)).sum(-1) if desc == "lpq" else np.minimum(p, q).sum(-1)
    best = np.sort(dist, axis=1)
    np.testing.assert_allclose([pr[1]["distances"][0] for pr in preds], best[:, 0], rtol=RTOL, atol=0)
    for pr, row, b in zip(preds, dist, best):
        if b[1] - b[0] > RTOL * b[0]:
            assert pr[0] == y[np.argmin(row)] and list(pr[1]["labels"]) == [y[np.argmin(row)]]
