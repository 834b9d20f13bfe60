"""Multi-scale LBP histograms (ofr_mslbp.hip) through CombineOperator: counts, float64 features, fp32 rows and
the model route against the float64 oracle (bytes) / a numpy restatement with the uint8 centre rule (floats),
concatenated per scale.  Everything is exact; distances 1e-10 relative against the fp64 chi-square of the
fp32-rounded histograms, as the project holds its fp32 histogram galleries.
"""
import functools

import facerec_oracle as O
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-10
# radii, P, n, H, W, grid, dtype ("const": a constant byte image)
CASES = [
    ((1, 2), 8, 2, 13, 18, (2, 3), np.uint8),         # smallest; uncovered margins differ per scale
    ((1, 2, 3), 8, 3, 20, 17, (2, 3), np.uint8),      # odd pitch, r1p8 form + generic forms in one launch
    ((1, 2, 3, 4), 8, 1, 40, 36, (2, 2), np.uint8),   # S = 4; cells > 255 pixels
    ((1, 2, 3), 8, 2, 40, 36, (14, 12), np.uint8),    # several bands; band row ranges differ per scale
    ((2, 2), 8, 1, 13, 18, (2, 3), np.uint8),         # equal radii; no r1p8 scale
    ((1, 3), 8, 2, 13, 18, (2, 3), np.float32),       # fp64 staging path
    ((1, 3), 8, 2, 18, 13, (2, 2), np.float64),
    ((1, 2), 8, 1, 40, 36, (1, 1), "const"),          # bin 2^P - 1 alone: the high half of a counter pair fills
    ((1, 2), 4, 2, 13, 18, (2, 3), np.uint8),
    ((1, 2), 6, 2, 13, 18, (2, 3), np.uint8),
]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    torch.cuda.set_device(0)


def combine(radii, P, grid):
    from ocvfacerec.facerec.feature import SpatialHistogram
    from ocvfacerec.facerec.lbp import ExtendedLBP
    from ocvfacerec.facerec.operators import CombineOperator
    ops = [SpatialHistogram(ExtendedLBP(r, P), grid) for r in radii]
    while len(ops) > 1:              # ((a, b), c), d
        ops[:2] = [CombineOperator(ops[0], ops[1])]
    return ops[0]


def elbp_float(X, radius, P):
    """lbp.py:80-130 on a float image: float64 arithmetic, the centre cast as (int64)trunc(x) & 255."""
    (oy, ox), (by, bx), offs, wts = O.elbp_geometry(radius, P)
    X = X.astype(np.float64)
    dy, dx = X.shape[0] - by + 1, X.shape[1] - bx + 1
    C = (np.trunc(X[oy:oy + dy, ox:ox + dx]).astype(np.int64) & 255).astype(np.float64)
    L = np.zeros((dy, dx), np.int64)
    for i, ((fy, fx, cy, cx), w) in enumerate(zip(offs, wts)):
        N = w[0] * X[fy:fy + dy, fx:fx + dx]
        N += w[1] * X[fy:fy + dy, cx:cx + dx]
        N += w[2] * X[cy:cy + dy, fx:fx + dx]
        N += w[3] * X[cy:cy + dy, cx:cx + dx]
        L += (N >= C).astype(np.int64) << i
    return L


def reference(x, radii, P, grid):
    """One face -> (counts [S][cells][2^P], float64 feature (1, N))."""
    C, F = [], []
    for r in radii:
        L = O.elbp(x, r, P) if x.dtype == np.uint8 else elbp_float(x, r, P)
        c, cell = O.spatial_histogram_counts(L, P, grid)
        C.append(c)
        F.append(c.reshape(-1) / float(cell))
    return np.stack(C), np.concatenate(F).reshape(1, -1)


@functools.lru_cache(maxsize=None)
def faces(n, H, W, dtype):
    if dtype == "const":
        return np.full((n, H, W), 77, np.uint8)
    X = np.random.default_rng(0).integers(0, 256, (n, H, W)).astype(np.uint8)
    return X if dtype == np.uint8 else X.astype(dtype) * dtype(0.37) + dtype(0.11)


@pytest.mark.parametrize("radii,P,n,H,W,grid,dtype", CASES)
def test_counts_and_rows(radii, P, n, H, W, grid, dtype):
    from ocvfacerec.facerec.operators import fused_scales
    from opencv_facerecognizer_amd import _device
    X = faces(n, H, W, dtype)
    op = combine(radii, P, grid)
    leaves = fused_scales(op, H, W)
    assert [f.lbp_operator.radius for f in leaves] == list(radii)
    ref = [reference(x, radii, P, grid) for x in X]
    C, F = np.stack([c for c, _ in ref]), np.stack([f for _, f in ref])
    counts, cells = op.counts_device(X)
    assert np.array_equal(_device.counts_numpy(counts, 2), C)
    if dtype == "const":
        assert (C[0, :, 0, -1] == cells).all() and C[0, :, 0, :-1].sum() == 0
    feats = op.compute(list(X), None)
    assert feats[0].dtype == np.float64 and feats[0].shape == (1, F.shape[2]) and np.array_equal(np.stack(feats), F)
    assert np.array_equal(op.extract(X[0]), F[0])
    Xd = torch.from_numpy(X).cuda()
    assert np.array_equal(op.density_batch(Xd).cpu().numpy(), F[:, 0].astype(np.float32))
    padded = _device.mslbp_hist(Xd, [f.lbp_operator.geometry() for f in leaves], grid, False, True, F.shape[2] + 8)[1]
    padded = padded.cpu().numpy()
    assert np.array_equal(padded[:, :-8], F[:, 0].astype(np.float32)) and not padded[:, -8:].any()


def test_not_fused():
    """Trees the kernel does not take: fused_scales is None, the answers are the hstack of the members' own."""
    from ocvfacerec.facerec.feature import SpatialHistogram
    from ocvfacerec.facerec.lbp import ExtendedLBP, OriginalLBP
    from ocvfacerec.facerec.operators import CombineOperator, fused_scales
    from opencv_facerecognizer_amd import _device
    from opencv_facerecognizer_amd._lib import E_UNSUPPORTED, OfrError

    def sh(r, P=8, grid=(2, 3)):
        return SpatialHistogram(ExtendedLBP(r, P), grid)
    small, big = faces(2, 13, 18, np.uint8), faces(1, 260, 260, np.uint8)
    trees = [(CombineOperator(sh(1, 8), sh(2, 6)), small), (CombineOperator(sh(1), sh(2, 8, (3, 2))), small),
             (combine((1, 2, 1, 2, 1), 8, (2, 3)), small), (combine((1, 2), 8, (1, 1)), big),
             (CombineOperator(sh(1), SpatialHistogram(OriginalLBP(), (2, 3))), small)]
    for op, X in trees:
        assert fused_scales(op, *X.shape[1:]) is None
        want = [np.hstack((np.asarray(a).reshape(1, -1), np.asarray(b).reshape(1, -1)))
                for a, b in zip(op.model1.compute(list(X), None), op.model2.compute(list(X), None))]
        for got in (op.compute(list(X), None), op.compute(X, None)):       # a list, an array [n][H][W]
            assert all(np.array_equal(g, w) and g.shape == w.shape for g, w in zip(got, want))
        assert np.array_equal(op.density_batch(X).cpu().numpy(), np.concatenate(want).astype(np.float32))
        assert np.array_equal(op.extract(X[0]), want[0])
    geoms = [ExtendedLBP(r, 8).geometry() for r in (1, 2, 1, 2, 1)]
    calls = [(small, geoms, (2, 3)), (big, geoms[:2], (1, 1)), (small, [ExtendedLBP(r, 9).geometry() for r in (1, 2)], (2, 3)),
             (small, geoms[:2], (10, 3))]         # five scales; cell of 66564; P = 9; radius 2 has 9 code rows
    for X, g, grid in calls:
        with pytest.raises(OfrError) as e:
            _device.mslbp_hist(torch.from_numpy(X).cuda(), g, grid)
        assert e.value.code == E_UNSUPPORTED
    with pytest.raises(TypeError):
        combine((1, 2), 8, (2, 3)).density_batch(torch.zeros((1, 13, 18), dtype=torch.int32).cuda())


def chi2(Q, G):
    p, q = Q[:, None, :], G[None, :, :]
    return ((p - q) ** 2 / (p + q + np.finfo("float").eps)).sum(-1)


@pytest.mark.parametrize("k,chain", [(1, False), (3, False), (1, True), (3, True)])
def test_model(k, chain, tmp_path):
    from ocvfacerec.facerec.classifier import NearestNeighbor
    from ocvfacerec.facerec.distance import ChiSquareDistance
    from ocvfacerec.facerec.model import PredictableModel
    from ocvfacerec.facerec.operators import ChainOperator
    from ocvfacerec.facerec.preprocessing import TanTriggsPreprocessing
    from ocvfacerec.facerec.serialization import load_model, save_model
    from opencv_facerecognizer_amd import _device, _lib
    X = list(faces(31, 18, 13, np.uint8))
    Xg, Q, y = X[:24], X[24:], np.arange(24) % 6
    pre = [TanTriggsPreprocessing().extract(x) for x in X] if chain else X
    H = np.concatenate([reference(x, (1, 2), 8, (2, 2))[1] for x in pre])
    H32 = H.astype(np.float32)
    feature = combine((1, 2), 8, (2, 2))
    model = PredictableModel(ChainOperator(TanTriggsPreprocessing(), feature) if chain else feature,
                             NearestNeighbor(ChiSquareDistance(), k))
    model.compute(Xg, y)
    g = model.classifier.__dict__["_dev"][2]          # the gallery compute left on the device
    assert isinstance(g, _device.Chi2Gallery) and g.dtype == _lib.DT_F32 and g is model.classifier._gallery()
    assert np.array_equal(g.G[:, :g.nbins].cpu().numpy(), H32[:24])
    assert np.array_equal(np.concatenate(model.classifier.X), H[:24])
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
