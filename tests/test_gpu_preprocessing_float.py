"""Tan-Triggs and histogram equalisation of float32 / float64 faces (ofr_preproc_float.hip) against plain
numpy / scipy restatements of reference preprocessing.py:98-105 and 73-77, and the batched route of a model
with a preprocessing chain against its one-face route.

Tan-Triggs: the float64 restatement runs on the float32-rounded input; the bound is 4 x the deviation of
the reference's own float32 run from it on the very inputs of each case (DEV32, measured once on a CPU
with numpy 2.2.6 / scipy 1.15.3).  Equalisation: np.histogram / np.interp on an array of the image's own
dtype, 1e-9 absolute on outputs in 0..255 (test_gpu_preprocessing.py's number and reasoning) -- the fp64
rounding of a cumsum and one interpolation stays orders of magnitude below it, one mis-binned pixel moves
the output by at least 255 / (H W) = 6e-3 at the largest face here.  Distances: 1e-10 relative.
"""
import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter

pytestmark = pytest.mark.gpu

RTOL = 1e-10
DEFAULT = (0.1, 10.0, 0.2, 1.0, 2.0)
# id -> n, H, W, dtype, (low, high) of the values, slice [1:] of the stack, DEV32
TT_CASES = {
    "5x6_shorter_than_both_radii": (1, 5, 6, np.float32, (0, 255), False, 5.654e-06),
    "9x70_wider_than_a_wave_f64": (1, 9, 70, np.float64, (0, 255), False, 1.123e-05),
    "3x70x36_means_per_face_small_values": (3, 70, 36, np.float32, (1e-3, 1), False, 5.408e-06),
    "113x113_resident_limit_f64": (1, 113, 113, np.float64, (1e-3, 1), False, 9.092e-06),
    "114x114_strips": (1, 114, 114, np.float32, (0, 255), False, 1.075e-05),
    "2_of_3x7x9_first_byte_unaligned": (3, 7, 9, np.float32, (0, 255), True, 6.124e-06),
}
# id -> n, H, W, dtype, num_bins, (low, high), constant
HE_CASES = {
    "13x18_f32_256": (1, 13, 18, np.float32, 256, (-10, 10), False),
    "13x18_f64_1024": (1, 13, 18, np.float64, 1024, (0, 255), False),
    "3x18x13_f32_64": (3, 18, 13, np.float32, 64, (0, 255), False),
    "3x18x13_f64_7": (3, 18, 13, np.float64, 7, (-10, 10), False),
    "210x200_f32_second_read_from_memory": (1, 210, 200, np.float32, 256, (-10, 10), False),
    "210x200_f64_second_read_from_memory": (1, 210, 200, np.float64, 64, (0, 255), False),
    "13x18_f32_constant": (1, 13, 18, np.float32, 256, (0, 255), True),
    "13x18_f64_constant": (1, 13, 18, np.float64, 7, (-10, 10), True),
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    torch.cuda.set_device(0)


def tantriggs_ref(img, alpha, tau, gamma, sigma0, sigma1, dtype=np.float64):
    X = np.power(np.array(img, dtype=dtype), gamma)
    X = gaussian_filter(X, sigma1) - gaussian_filter(X, sigma0)
    X = X / np.power(np.mean(np.power(np.abs(X), alpha)), 1.0 / alpha)
    X = X / np.power(np.mean(np.power(np.minimum(np.abs(X), tau), alpha)), 1.0 / alpha)
    return tau * np.tanh(X / tau)


def histeq_ref(img, num_bins):
    h, b = np.histogram(img.flatten(), num_bins, density=True)
    cdf = h.cumsum()
    cdf = 255 * cdf / cdf[-1]
    return np.interp(img.flatten(), b[:-1], cdf).reshape(img.shape)


def tt_input(case):
    n, H, W, dtype, (low, high), _, _ = TT_CASES[case]
    rng = np.random.default_rng(sorted(TT_CASES).index(case))
    return rng.uniform(low, high, size=(n, H, W)).astype(dtype)


@pytest.mark.parametrize("case", list(TT_CASES))
def test_tantriggs_matches_float64(case):
    from ocvfacerec.facerec.preprocessing import TanTriggsPreprocessing
    n, H, W, dtype, _, sliced, dev32 = TT_CASES[case]
    X = tt_input(case)
    Xd = torch.from_numpy(X).cuda()
    if sliced:
        X, Xd, n = X[1:], Xd[1:], n - 1
        assert Xd.data_ptr() % 16 != 0
    ref = np.stack([tantriggs_ref(x.astype(np.float32), *DEFAULT) for x in X])
    assert np.isfinite(ref).all()
    op = TanTriggsPreprocessing(*DEFAULT)
    got = op.extract_batch(Xd)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, H, W)
    got = got.cpu().numpy()
    err = np.abs(got - ref).max()
    print(f"{case}: max |kernel - float64| = {err:.3e}, bound 4 x {dev32:.3e}")
    assert err <= 4 * dev32
    one = op.extract(X[n - 1])                      # a face's result does not depend on its batch
    assert one.dtype == np.float32 and np.array_equal(one, got[n - 1])


@pytest.mark.parametrize("case", list(HE_CASES))
def test_histeq_matches_numpy_on_the_same_dtype(case):
    from ocvfacerec.facerec.preprocessing import HistogramEqualization
    n, H, W, dtype, num_bins, (low, high), constant = HE_CASES[case]
    rng = np.random.default_rng(sorted(HE_CASES).index(case))
    X = rng.uniform(low, high, size=(n, H, W)).astype(dtype)
    if constant:
        X[:] = X[0, 0, 0]
    else:
        for x in X:                                 # pixels exactly on interior bin edges, numpy's own
            edges = np.histogram(x.flatten(), num_bins)[1]
            assert edges.dtype == dtype
            inner = np.flatnonzero((x.flat != x.min()) & (x.flat != x.max()))
            pos = rng.choice(inner, size=H * W // 6, replace=False)
            x.flat[pos] = edges[rng.integers(1, num_bins, size=pos.size)]
    ref = np.stack([histeq_ref(x, num_bins) for x in X])
    assert np.isfinite(ref).all()
    got = HistogramEqualization(num_bins).extract_batch(torch.from_numpy(X).cuda())
    assert got.dtype == torch.float64 and tuple(got.shape) == (n, H, W)
    err = np.abs(got.cpu().numpy() - ref).max()
    print(f"{case}: max |kernel - numpy| = {err:.3e}")
    assert err <= 1e-9


@pytest.mark.parametrize("device_input", [False, True])
@pytest.mark.parametrize("route", ["lbph", "fisherfaces"])
def test_preprocessing_chain_batched_route_matches_one_face_route(route, device_input):
    from ocvfacerec.facerec.classifier import NearestNeighbor
    from ocvfacerec.facerec.distance import ChiSquareDistance, EuclideanDistance
    from ocvfacerec.facerec.feature import Fisherfaces, SpatialHistogram
    from ocvfacerec.facerec.model import PredictableModel
    from ocvfacerec.facerec.operators import ChainOperator
    from ocvfacerec.facerec.preprocessing import HistogramEqualization, TanTriggsPreprocessing
    rng = np.random.default_rng(7)
    y = np.repeat(np.arange(3), 4)
    proto = rng.integers(30, 226, size=(3, 16, 16))
    X = np.clip(proto[y] + rng.integers(-30, 31, size=(12, 16, 16)), 0, 255).astype(np.uint8)
    pre = ChainOperator(TanTriggsPreprocessing(), HistogramEqualization())
    if route == "lbph":
        model = PredictableModel(ChainOperator(pre, SpatialHistogram()), NearestNeighbor(ChiSquareDistance()))
    else:
        model = PredictableModel(ChainOperator(pre, Fisherfaces()), NearestNeighbor(EuclideanDistance()))
    model.compute(list(X), y)
    assert model._lbph_chain() if route == "lbph" else model._chain()
    Q = np.clip(proto[y] + rng.integers(-30, 31, size=(12, 16, 16)), 0, 255).astype(np.uint8)
    one = [model.predict(x) for x in Q]
    got = model.predict_batch(torch.from_numpy(Q).cuda() if device_input else list(Q))
    assert [g[0] for g in got] == [o[0] for o in one]
    d_got = np.array([g[1]["distances"][0] for g in got])
    d_one = np.array([o[1]["distances"][0] for o in one])
    assert np.all(np.abs(d_got - d_one) <= RTOL * np.abs(d_one))
