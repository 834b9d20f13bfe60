"""Tan-Triggs and histogram equalisation (reference preprocessing.py:98-105, 73-77) on the GPU against plain
float64 restatements on the host, and the batched ChainOperator(TanTriggs, Fisherfaces) route of
PredictableModel against the one-face route.

Equalisation: 1e-9 absolute on outputs in 0..255 -- fp64 rounding over a cumsum of <= 256 terms and one
interpolation stays below 2e-11, one mis-binned pixel moves the output by at least 255 / (H W) = 3.4e-3 at
the largest face here.  Tan-Triggs: 4 x the deviation the reference's own float32 run has from the
float64 restatement on the very inputs of each case (DEV32, measured once on a CPU with numpy 2.2.6 /
scipy 1.15.3).  Distances: 1e-10 relative.
"""
import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter

pytestmark = pytest.mark.gpu

RTOL = 1e-10
RANGES = ((0, 256), (40, 200), (100, 140))      # value range of face i of a case
DEFAULT = (0.1, 10.0, 0.2, 1.0, 2.0)
# id -> n, H, W, (alpha, tau, gamma, sigma0, sigma1), DEV32 = max |float32 reference - float64 restatement|
TT_CASES = {
    "5x6_shorter_than_both_radii": (1, 5, 6, DEFAULT, 8.781e-06),
    "13x18": (1, 13, 18, DEFAULT, 1.220e-03),
    "18x13": (1, 18, 13, DEFAULT, 7.150e-06),
    "9x70_wider_than_a_wave": (1, 9, 70, DEFAULT, 7.019e-06),
    "3x70x36_means_per_face": (3, 70, 36, DEFAULT, 5.710e-05),
    "200x168_strips": (1, 200, 168, DEFAULT, 7.590e-06),
    "128x128_resident_limit": (2, 128, 128, DEFAULT, 1.547e-05),
    "40x36_radii_2_and_12": (1, 40, 36, (0.2, 5.0, 0.5, 0.5, 3.0), 1.372e-06),
}
# id -> n, H, W, num_bins, constant
HE_CASES = {
    "13x18_full_range_256": (1, 13, 18, 256, False),
    "3x18x13_64": (3, 18, 13, 64, False),
    "40x36_7": (1, 40, 36, 7, False),
    "13x18_constant": (1, 13, 18, 256, True),
    "200x168_256": (1, 200, 168, 256, False),
    "300x250_1024_second_read_from_memory": (1, 300, 250, 1024, False),
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


@pytest.mark.parametrize("case", list(TT_CASES))
def test_tantriggs_matches_float64(case):
    from ocvfacerec.facerec.preprocessing import TanTriggsPreprocessing
    n, H, W, params, dev32 = TT_CASES[case]
    rng = np.random.default_rng(sorted(TT_CASES).index(case))
    X = np.stack([rng.integers(*RANGES[i], size=(H, W)) for i in range(n)]).astype(np.uint8)
    ref = np.stack([tantriggs_ref(x, *params) for x in X])
    assert np.isfinite(ref).all()
    op = TanTriggsPreprocessing(*params)
    got = op.extract_batch(torch.from_numpy(X).cuda())
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, H, W)
    got = got.cpu().numpy()
    err = np.abs(got - ref).max()
    print(f"{case}: max |kernel - float64| = {err:.3e}, bound 4 x {dev32:.3e}")
    assert err <= 4 * dev32
    one = op.extract(X[n - 1])                      # a face's result does not depend on its batch
    assert one.dtype == np.float32 and np.array_equal(one, got[n - 1])


@pytest.mark.parametrize("case", list(HE_CASES))
def test_histeq_matches_numpy(case):
    from ocvfacerec.facerec.preprocessing import HistogramEqualization
    n, H, W, num_bins, constant = HE_CASES[case]
    rng = np.random.default_rng(sorted(HE_CASES).index(case))
    X = np.stack([rng.integers(*RANGES[i], size=(H, W)) for i in range(n)]).astype(np.uint8)
    if constant:
        X[:] = 77
    else:
        X[0, 0, :2] = (0, 255)                      # face 0 spans the full range: bin width 255 / num_bins
    ref = np.stack([histeq_ref(x, num_bins) for x in X])
    assert np.isfinite(ref).all()
    got = HistogramEqualization(num_bins).compute(list(X), None)
    assert all(g.dtype == np.float64 and g.shape == (H, W) for g in got)
    err = np.abs(np.stack(got) - ref).max()
    print(f"{case}: max |kernel - numpy| = {err:.3e}")
    assert err <= 1e-9


@pytest.mark.parametrize("device_input", [False, True])
def test_chain_batched_route_matches_one_face_route(device_input):
    from ocvfacerec.facerec.classifier import NearestNeighbor
    from ocvfacerec.facerec.distance import EuclideanDistance
    from ocvfacerec.facerec.feature import Fisherfaces
    from ocvfacerec.facerec.model import PredictableModel
    from ocvfacerec.facerec.operators import ChainOperator
    from ocvfacerec.facerec.preprocessing import TanTriggsPreprocessing
    rng = np.random.default_rng(7)
    y = np.repeat(np.arange(3), 4)
    proto = rng.integers(30, 226, size=(3, 16, 16))
    X = np.clip(proto[y] + rng.integers(-30, 31, size=(12, 16, 16)), 0, 255).astype(np.uint8)
    model = PredictableModel(ChainOperator(TanTriggsPreprocessing(), Fisherfaces()), NearestNeighbor(EuclideanDistance(), k=1))
    model.compute(list(X), y)
    assert model._chain()
    Q = np.clip(proto[y] + rng.integers(-30, 31, size=(12, 16, 16)), 0, 255).astype(np.uint8)
    one = [model.predict(x) for x in Q]
    got = model.predict_batch(torch.from_numpy(Q).cuda() if device_input else list(Q))
    assert [g[0] for g in got] == [o[0] for o in one]
    d_got = np.array([g[1]["distances"][0] for g in got])
    d_one = np.array([o[1]["distances"][0] for o in one])
    assert np.all(np.abs(d_got - d_one) <= RTOL * np.abs(d_one))
    feats = model.feature.extract_batch(list(Q)).cpu().numpy()
    assert np.allclose(feats, np.stack([np.asarray(model.feature.extract(x)).reshape(-1) for x in Q]), rtol=0,
                       atol=RTOL * np.abs(feats).max())
    with pytest.raises(TypeError):
        model.feature.model2.project_device(torch.zeros((2, 16, 16), dtype=torch.int32, device="cuda"))
