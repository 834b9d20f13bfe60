"""NormalizedCorrelation (reference distance.py:80-98) through NearestNeighbor on the GPU, against the
formula in numpy float64.

Tolerance 1e-11 absolute: three fp64 sums of <= 4160 terms, each within nbins 2^-53 ~ 4.6e-13 of quantities
that are <= 1 after normalisation, on both sides: under 3e-12.  Exact ties are common in integer data, so a
returned row may differ from the stable argsort when its distance is within the tolerance of the expected one.

Certification: in the u8 / u8hi cases with k <= 8 the smallest gap between the k-th and the 16th exact
distance over all queries is 3.0e-3 .. 4.4e-2 (numpy, these seeds), far above the MFMA pass's bound near 2^-23:
it must answer every query alone, last_fallbacks == (0,).
"""
import functools

import numpy as np
import pytest
import torch

from opencv_facerecognizer_amd import _lib

pytestmark = pytest.mark.gpu

ATOL = 1e-11
# kind, B, N, nbins, k
CASES = [("u8", 1, 5, 16, 1),         # one partial tile, N < 16
         ("u8", 33, 300, 64, 3),      # three gallery tiles, a partial query tile
         ("u8", 70, 300, 80, 8),      # a k tail: bins no multiple of the k step
         ("u8", 3, 130, 4160, 2),     # many k steps plus a tail
         ("u8hi", 33, 300, 200, 5), ("u8hi", 9, 260, 128, 8),   # counts up to ~190: the -128 re-centring
         ("u8", 5, 100, 64, 40),      # k > 16: the deep pass
         ("u16", 9, 150, 48, 4), ("f32", 9, 150, 50, 4),
         ("f32", 20, 140, 200, 5)]    # several stages plus a tail in the general kernel


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    torch.cuda.set_device(0)


def reference(Q, G):
    """distance.py:92-98 for every (query, row) pair, float64 [B][N]; NaN for a constant row."""
    Qc, Gc = Q - Q.mean(1, keepdims=True), G - G.mean(1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 1.0 - (Qc @ Gc.T) / (np.sqrt((Qc * Qc).sum(1))[:, None] * np.sqrt((Gc * Gc).sum(1))[None, :])


@functools.lru_cache(maxsize=None)
def rows(kind, B, N, nbins):
    """Float64 histogram rows (queries, gallery, expected distances): counts / cell pixels of 64-bin cells,
    the seeds and the u8 / u16 / f32 kinds of test_gpu_hist_metrics.rows; "u8hi": 255-pixel cells with one
    random dominant bin of probability 0.65 per (row, cell)."""
    r = np.random.Generator(np.random.PCG64(1000 * nbins + N))
    cells = [min(64, nbins - c) for c in range(0, nbins, 64)]
    if kind == "u16":
        pix, prob = 6000, [0.8 ** np.arange(c) / (0.8 ** np.arange(c)).sum() for c in cells]
    elif kind == "u8hi":
        pix, prob = 255, []
        for c in cells:
            p = np.full((B + N, c), 0.35 / (c - 1))
            p[np.arange(B + N), r.integers(0, c, B + N)] = 0.65
            prob.append(p)
    else:
        pix, prob = 64, [np.full(c, 1.0 / c) for c in cells]
    C = np.concatenate([r.multinomial(pix, pr, size=None if kind == "u8hi" else B + N) for pr in prob],
                       axis=1).astype(np.float64)
    if kind == "f32":
        C = ((C + r.random(C.shape)) / pix).astype(np.float32).astype(np.float64) * pix
    Q, G = C[:B] / pix, C[B:] / pix
    return Q, G, reference(Q, G)


def check_topk(D, d, i):
    k = d.shape[1]
    at = np.take_along_axis(D, i, axis=1)
    np.testing.assert_allclose(d, at, rtol=0, atol=ATOL)
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    want = np.take_along_axis(D, order, axis=1)
    off = i != order
    assert (np.abs(at - want)[off] <= ATOL).all(), (i[off], order[off])


def _nn(k):
    from ocvfacerec.facerec.classifier import NearestNeighbor
    from ocvfacerec.facerec.distance import NormalizedCorrelation
    return NearestNeighbor(NormalizedCorrelation(), k=k)


@pytest.mark.parametrize("kind,B,N,nbins,k", CASES)
def test_search_matches_numpy(kind, B, N, nbins, k):
    Q, G, D = rows(kind, B, N, nbins)
    nn = _nn(k)
    nn.compute(list(G), np.arange(N))
    d, i = nn.search(Q)
    g = nn._gallery()
    assert g.dtype == {"u8": _lib.DT_U8, "u8hi": _lib.DT_U8, "u16": _lib.DT_U16, "f32": _lib.DT_F32}[kind]
    assert g.metric == _lib.METRIC_NCORR and d.shape == (B, k) and (i >= 0).all() and (i < N).all()
    if kind == "u8hi":
        assert int(g.G.max()) > 128
    check_topk(D, d, i)
    if kind in ("u8", "u8hi") and k <= 8:
        assert g.last_fallbacks == (0,)   # see the module docstring


def test_ties_force_exact_pass():
    """The best row repeated 20 times: the 16 candidates tie, nothing certifies, the exact pass returns the
    lowest rows of the run."""
    _, G, _ = rows("u8", 33, 300, 64)
    G = G[:60].copy()
    G[10:30] = G[10]
    Q = np.repeat(G[10:11], 4, axis=0)
    Q[np.arange(4), np.arange(4)] += 1 / 64    # four different queries, each nearest to the repeated row
    nn = _nn(3)
    nn.compute(list(G), np.arange(60))
    d, i = nn.search(Q)
    assert nn._gallery().last_fallbacks[0] == 4
    assert (i == [10, 11, 12]).all()
    check_topk(reference(Q, G), d, i)


def test_constant_rows_rank_last():
    Q, G, _ = rows("u8", 1, 5, 16)
    Q, G = np.concatenate([Q, np.full((1, 16), 4 / 64)]), np.concatenate([G, G[:1]])
    G[2] = 4 / 64
    nn = _nn(6)
    nn.compute(list(G), np.arange(6))
    d, i = nn.search(Q)
    assert nn._gallery().dtype == _lib.DT_U8
    assert i[0, 5] == 2 and np.isnan(d[0, 5])
    D = reference(Q[:1], G)
    np.testing.assert_allclose(d[0, :5], np.sort(D[0][~np.isnan(D[0])]), rtol=0, atol=ATOL)
    assert np.isnan(d[1]).all() and (i[1] == np.arange(6)).all()


def test_single_pair():
    from ocvfacerec.facerec.distance import NormalizedCorrelation
    Q, G, D = rows("u8", 33, 300, 64)
    assert abs(NormalizedCorrelation()(Q[0], G[0]) - D[0, 0]) <= ATOL
    assert abs(NormalizedCorrelation()(3 * Q[0] + 5, Q[0])) <= ATOL


def test_lbph_model():
    from ocvfacerec.facerec.classifier import vote
    from ocvfacerec.facerec.feature import SpatialHistogram
    from ocvfacerec.facerec.lbp import ExtendedLBP
    from ocvfacerec.facerec.model import PredictableModel
    r = np.random.Generator(np.random.PCG64(5))
    X = list(r.integers(0, 256, (40, 64, 64)).astype(np.uint8))
    y = np.arange(40) % 10
    model = PredictableModel(SpatialHistogram(ExtendedLBP(1, 8), (8, 8)), _nn(3))
    model.compute(X, y)
    assert model.classifier._gallery().dtype == _lib.DT_U8   # the adopted device counts
    H = np.stack([np.asarray(h, np.float64).reshape(-1) for h in model.classifier.X])
    preds = model.predict_batch(X[:5])
    D = reference(H[:5], H)
    d = np.array([p[1]["distances"] for p in preds])
    order = np.argsort(D, axis=1, kind="stable")[:, :3]
    np.testing.assert_allclose(d, np.take_along_axis(D, order, axis=1), rtol=0, atol=ATOL)
    for p, o, row in zip(preds, order, D):
        if (np.diff(np.sort(row)[:4]) > ATOL).all():
            assert list(p[1]["labels"]) == list(y[o]) and p[0] == vote(y[o])
