"""preprocessing without a device: the reference's module path, repr strings, pickled attribute names, and
the argument checks of the C entry points (made before any device work)."""
from opencv_facerecognizer_amd import _lib
from ocvfacerec.facerec.lbp import ExtendedLBP
from ocvfacerec.facerec.preprocessing import HistogramEqualization, LBPPreprocessing, TanTriggsPreprocessing
from ocvfacerec.facerec.serialization import dumps_model, loads_model


def test_repr_strings():
    assert repr(TanTriggsPreprocessing()) == \
        "TanTriggsPreprocessing (alpha=0.100,tau=10.000,gamma=0.200,sigma0=1.000,sigma1=2.000)"
    assert repr(HistogramEqualization(64)) == "HistogramEqualization (num_bins=64)"
    assert repr(LBPPreprocessing()) == "LBPPreprocessing (lbp_operator=ExtendedLBP (neighbors=8, radius=1))"


def test_pickle_round_trip_keeps_reference_names():
    tt = TanTriggsPreprocessing(0.2, 5, 0.5, 0.5, 3)
    for op, state in ((tt, {"_alpha": 0.2, "_tau": 5.0, "_gamma": 0.5, "_sigma0": 0.5, "_sigma1": 3.0}),
                      (HistogramEqualization(7), {"_num_bins": 7})):
        data = dumps_model(op)
        assert b"ocvfacerec.facerec.preprocessing" in data and type(op).__name__.encode() in data
        back = loads_model(data)
        assert type(back) is type(op) and back.__dict__ == state
    back = loads_model(dumps_model(LBPPreprocessing(ExtendedLBP(2, 6))))
    assert list(back.__dict__) == ["_lbp_operator"] and back._lbp_operator.radius == 2


def test_error_paths_without_device():
    lib = _lib.load()

    def tt(alpha=0.1, tau=10.0, gamma=0.2, s0=1.0, s1=2.0):
        return lib.ofr_tantriggs_f32(None, None, 1, 16, 16, alpha, tau, gamma, s0, s1, None, None, 0)
    for bad, word in (({"alpha": 0.0}, b"alpha"), ({"tau": -1.0}, b"tau"), ({"s0": 0.0}, b"sigma"), ({"s1": 4.2}, b"radius")):
        assert tt(**bad) == -1 and word in lib.ofr_last_error()
    assert tt(s1=4.1) == -1 and b"null" in lib.ofr_last_error()      # radius 16 is served
    for nb in (0, 4097):
        assert lib.ofr_histeq_f64(None, None, 1, 16, 16, nb, None) == -1 and b"num_bins" in lib.ofr_last_error()
    assert lib.ofr_tantriggs_workspace_bytes(4, 128, 128, 1.0, 2.0) == 0     # resident: no workspace
    assert lib.ofr_tantriggs_workspace_bytes(4, 200, 168, 1.0, 2.0) > 0      # strips: per-strip partial sums
