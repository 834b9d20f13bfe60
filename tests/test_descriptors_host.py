"""OriginalLBP and LPQ without a device: reference names in pickles, repr strings, argument checks of the
C entry points (before any device work, as tests/test_abi.py::test_error_paths_without_device)."""
import numpy as np

from opencv_facerecognizer_amd import _lib
from ocvfacerec.facerec.feature import SpatialHistogram
from ocvfacerec.facerec.lbp import LPQ, OriginalLBP
from ocvfacerec.facerec.serialization import dumps_model, loads_model


def test_pickle_round_trip_under_reference_names():
    for op in (LPQ(2), OriginalLBP()):
        data = dumps_model(SpatialHistogram(op, (4, 5)))
        assert b"ocvfacerec.facerec.lbp" in data and type(op).__name__.encode() in data
        back = loads_model(data)
        assert type(back.lbp_operator) is type(op) and back.sz == (4, 5)
        assert back.lbp_operator.__dict__ == op.__dict__ and back.lbp_operator.neighbors == 8
    assert back.lbp_operator.__dict__ == {"_neighbors": 8}
    assert loads_model(dumps_model(LPQ(2))).radius == 2


def test_repr_strings():
    assert repr(OriginalLBP()) == "OriginalLBP (neighbors=8)"
    assert repr(LPQ()) == "LPQ (neighbors=8, radius=3)"
    assert repr(SpatialHistogram(LPQ(2), (4, 4))) == "SpatialHistogram (operator=LPQ (neighbors=8, radius=2), grid=(4, 4))"


def test_error_paths_without_device():
    lib = _lib.load()
    V = np.eye(8).ctypes.data_as(_lib.c_vp)
    for r, rc, word in ((0, -1, b"radius"), (9, -2, b"radius")):
        assert lib.ofr_lpq_codes(None, None, 1, 16, 16, r, V, None) == rc and word in lib.ofr_last_error()
        assert lib.ofr_lpq_hist(None, None, 1, 16, 16, r, V, 2, 2, None, 1) == rc and word in lib.ofr_last_error()
    assert lib.ofr_lpq_codes(None, None, 1, 16, 16, 3, None, None) == -1 and b"basis" in lib.ofr_last_error()
    assert lib.ofr_lpq_hist(None, None, 1, 16, 16, 3, V, 17, 2, None, 1) == -1 and b"grid" in lib.ofr_last_error()
    assert lib.ofr_olbp_hist(None, None, 1, 16, 16, 2, 15, None, 1) == -1 and b"grid" in lib.ofr_last_error()
    assert lib.ofr_lpq_hist(None, None, 1, 40, 36, 3, V, 2, 2, None, 1) == -1 and b"count_bytes" in lib.ofr_last_error()
    assert lib.ofr_olbp_hist(None, None, 1, 40, 36, 2, 2, None, 3) == -1 and b"count_bytes" in lib.ofr_last_error()
    for rc in (lib.ofr_lpq_codes(None, None, 1, 16, 16, 3, V, None), lib.ofr_lpq_hist(None, None, 1, 16, 16, 3, V, 2, 2, None, 1),
               lib.ofr_olbp_codes(None, None, 1, 16, 16, None), lib.ofr_olbp_hist(None, None, 1, 16, 16, 2, 2, None, 1)):
        assert rc == -1 and b"null pointer" in lib.ofr_last_error()
    assert lib.ofr_lpq_hist(None, None, 0, 16, 16, 3, V, 2, 2, None, 1) == 0 and lib.ofr_olbp_codes(None, None, 0, 16, 16, None) == 0
