"""VarLBP (ofr_varlbp.hip): variance image, fused cell counts + per-cell totals, the fp32 density rows and the
model route, against a float64 numpy restatement of lbp.py:140-208 / feature.py:286-302.

Everything is exact: the variance image bit for bit, counts and totals as integers, features as counts / totals
(NaN bins for a cell with nothing in range).  Distances: 1e-10 relative against the fp64 chi-square of the
fp32-rounded histograms, as tests/test_gpu_hist_metrics.py holds its f32 galleries.
Default input: default_rng(0).integers(100, 148): 1-2 % of the variances above 2^P, none on an integer edge.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-10
EPS = np.finfo("float").eps
GEOMS = [(1, 8), (2, 8), (3, 12), (2, 6), (1, 4)]
DTYPES = [np.uint8, np.float32, np.float64]
# r, P, n, H, W, grid, dtype
HIST_CASES = [
    (1, 8, 2, 13, 18, (2, 3), np.uint8),     # smallest ordinary case
    (1, 8, 3, 18, 13, (2, 2), np.uint8),     # odd pitch
    (2, 8, 1, 40, 36, (2, 2), np.uint8),     # cell 288: 16-bit counts
    (1, 8, 2, 40, 36, (9, 9), np.uint8),     # two bands
    (1, 8, 2, 40, 36, (14, 12), np.uint8),   # 168 cells: more counters than LDS holds
    (3, 12, 1, 40, 36, (2, 2), np.uint8),    # 4096 bins
    (2, 6, 1, 23, 29, (3, 2), np.uint8),     # about 90 % of the values dropped
    (1, 4, 1, 13, 18, (2, 3), np.uint8),     # one cell ends empty: NaN bins
    (3, 12, 2, 40, 36, (2, 12), np.uint8),   # 12 x 4096 counters: one cell row exceeds LDS, global counters
    (1, 8, 2, 13, 18, (2, 3), np.float32),
    (2, 8, 2, 18, 13, (2, 2), np.float64),
]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    torch.cuda.set_device(0)


def var_ref(X, radius, P):
    from ocvfacerec.facerec.lbp import elbp_geometry
    (oy, ox), (by, bx), offs, wts = elbp_geometry(radius, P)
    X = X.astype(np.float64)
    dy, dx = max(X.shape[0] - by + 1, 0), max(X.shape[1] - bx + 1, 0)
    mean, m2 = np.zeros((dy, dx)), np.zeros((dy, dx))
    for i, ((fy, fx, cy, cx), w) in enumerate(zip(offs, wts)):
        N = None
        for (ty, tx), wt in zip(((fy, fx), (fy, cx), (cy, fx), (cy, cx)), w):
            if wt != 0.0:
                term = wt * X[ty:ty + dy, tx:tx + dx]
                N = term if N is None else N + term
        delta = N - mean
        mean = mean + delta / float(i + 1)
        m2 = m2 + delta * (N - mean)
    return m2 / (P - 1)


@functools.lru_cache(maxsize=None)
def case(radius, P, dtype, n, H, W, nan=False):
    """Images and their reference variance images, computed once per shape."""
    X = np.random.default_rng(0).integers(100, 148, (n, H, W)).astype(np.uint8)
    if dtype != np.uint8:
        X = X.astype(dtype) * dtype(0.37) + dtype(0.11)
        assert X.dtype == dtype
    if nan:
        X[0, H // 2, W // 2] = np.nan
    with np.errstate(invalid="ignore"):
        return X, np.stack([var_ref(x, radius, P) for x in X])


def cell_counts(V, grid, P):
    """feature.py:286-302 as integers: counts [cells][2^P] and the in-range total of every cell."""
    py, px = V.shape[0] // grid[0], V.shape[1] // grid[1]
    with np.errstate(invalid="ignore"):
        C = np.array([np.histogram(V[r * py:(r + 1) * py, c * px:(c + 1) * px], bins=2 ** P, range=(0, 2 ** P))[0]
                      for r in range(grid[0]) for c in range(grid[1])])
    return C, C.sum(1)


def density(C, T):
    with np.errstate(invalid="ignore"):
        return (C / T[..., None].astype(np.float64)).reshape(C.shape[:-2] + (-1,))


@pytest.mark.parametrize("n,H,W", [(1, 13, 18), (1, 18, 13), (3, 40, 36)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("radius,P", GEOMS + [(1, 32)])
def test_variance_image(radius, P, dtype, n, H, W):
    from ocvfacerec.facerec.lbp import VarLBP
    X, want = case(radius, P, dtype, n, H, W)
    op = VarLBP(radius, P)
    got = op.values_batch(torch.from_numpy(X).cuda()).cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, want)
    one = op(X[0])
    assert one.dtype == np.float64 and np.array_equal(one, want[0])


@pytest.mark.parametrize("dtype,H,W", [(np.uint8, 3, 3), (np.float32, 3, 3),    # a 1 x 1 result
                                       (np.uint8, 3, 21000), (np.float64, 4, 7000)])   # three rows exceed LDS
def test_variance_image_edges(dtype, H, W):
    from ocvfacerec.facerec.lbp import VarLBP
    from ocvfacerec.facerec.preprocessing import LBPPreprocessing
    X, want = case(1, 8, dtype, 1, H, W)
    assert np.array_equal(LBPPreprocessing(VarLBP()).extract(X[0]), want[0])


@pytest.mark.parametrize("radius,P,n,H,W,grid,dtype", HIST_CASES + [(1, 8, 2, 13, 18, (2, 3), "nan")])
def test_fused_histogram(radius, P, n, H, W, grid, dtype):
    from ocvfacerec.facerec.feature import SpatialHistogram
    from ocvfacerec.facerec.lbp import VarLBP
    from opencv_facerecognizer_amd._device import counts_numpy
    X, V = case(radius, P, np.float32, n, H, W, nan=True) if dtype == "nan" else case(radius, P, dtype, n, H, W)
    ref = [cell_counts(v, grid, P) for v in V]
    C, T = np.stack([c for c, _ in ref]), np.stack([t for _, t in ref])
    assert (T == 0).any() == ((radius, P) == (1, 4))          # the empty cell, and only there
    sh = SpatialHistogram(VarLBP(radius, P), grid)
    counts, totals, cb = sh.counts_device(X)
    assert np.array_equal(counts_numpy(counts, cb), C) and np.array_equal(totals.cpu().numpy(), T)
    Href = density(C, T)
    feats = sh.compute(list(X), None)
    assert np.array_equal(np.stack(feats), Href, equal_nan=True) and feats[0].dtype == np.float64
    assert np.array_equal(sh.extract(X[0]), Href[0], equal_nan=True)
    rows = sh.density_batch(torch.from_numpy(X).cuda()).cpu().numpy()
    assert rows.dtype == np.float32 and np.array_equal(rows, Href.astype(np.float32), equal_nan=True)


def chi2(Q, G):
    p, q = Q[:, None, :], G[None, :, :]
    return ((p - q) ** 2 / (p + q + EPS)).sum(-1)


@pytest.mark.parametrize("k,chain", [(1, False), (3, False), (3, True)])
def test_model(k, chain, tmp_path):
    from ocvfacerec.facerec.classifier import NearestNeighbor
    from ocvfacerec.facerec.distance import ChiSquareDistance
    from ocvfacerec.facerec.feature import SpatialHistogram
    from ocvfacerec.facerec.lbp import VarLBP
    from ocvfacerec.facerec.model import PredictableModel
    from ocvfacerec.facerec.operators import ChainOperator
    from ocvfacerec.facerec.preprocessing import TanTriggsPreprocessing
    from ocvfacerec.facerec.serialization import load_model, save_model
    from opencv_facerecognizer_amd import _device, _lib
    faces = list(np.random.default_rng(0).integers(100, 148, (31, 18, 13)).astype(np.uint8))
    X, Q, y = faces[:24], faces[24:], np.arange(24) % 6
    feature = SpatialHistogram(VarLBP(), (2, 2))
    pre = [TanTriggsPreprocessing().extract(x) for x in faces] if chain else faces
    H = np.stack([density(*cell_counts(var_ref(x, 1, 8), (2, 2), 8)) for x in pre])
    H32 = H.astype(np.float32)
    model = PredictableModel(ChainOperator(TanTriggsPreprocessing(), feature) if chain else feature,
                             NearestNeighbor(ChiSquareDistance(), k))
    model.compute(X, y)
    g = model.classifier.__dict__["_dev"][2]          # the gallery compute left on the device
    assert isinstance(g, _device.Chi2Gallery) and g.dtype == _lib.DT_F32 and g is model.classifier._gallery()
    assert np.array_equal(g.G[:, :g.nbins].cpu().numpy(), H32[:24])
    assert np.array_equal(np.stack(model.classifier.X), H[:24])
    d, i = model.search_batch(Q, k)
    D = chi2(H32[24:].astype(np.float64), H32[:24].astype(np.float64))
    at, order = np.take_along_axis(D, i, axis=1), np.argsort(D, axis=1, kind="stable")[:, :k]
    np.testing.assert_allclose(d, at, rtol=RTOL, atol=0)
    want = np.take_along_axis(D, order, axis=1)
    off = i != order
    assert (np.abs(at - want)[off] <= RTOL * np.abs(want)[off]).all(), (i[off], order[off])
    batch, single = model.predict_batch(Q), [model.predict(x) for x in Q]
    save_model(str(tmp_path / "m.pkl"), model)
    loaded = load_model(str(tmp_path / "m.pkl")).predict_batch(Q)
    for b, s, l in zip(batch, single, loaded):
        for other in (s, l):
            assert b[0] == other[0] and np.array_equal(b[1]["labels"], other[1]["labels"])
            assert np.array_equal(b[1]["distances"], other[1]["distances"])


def test_errors():
    from ocvfacerec.facerec.feature import SpatialHistogram
    from ocvfacerec.facerec.lbp import ExtendedLBP, VarLBP
    from opencv_facerecognizer_amd._lib import E_UNSUPPORTED, OfrError
    X = case(1, 8, np.uint8, 2, 13, 18)[0]
    for op in (ExtendedLBP(1, 16), VarLBP(1, 16)):
        with pytest.raises(OfrError, match="neighbors must be <= 15") as e:
            SpatialHistogram(op, (2, 2)).extract(X[0])
        assert e.value.code == E_UNSUPPORTED
    with pytest.raises(OfrError, match="neighbors must be >= 2") as e:
        VarLBP(1, 1)(X[0])
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="density_batch"):
        SpatialHistogram(VarLBP(), (2, 2)).counts_batch(X)
