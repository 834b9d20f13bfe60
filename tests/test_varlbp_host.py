"""VarLBP without a GPU: the class as the reference's pickles name it, and the C entry points' argument checks."""
import numpy as np
import pytest


def test_class_surface_and_pickle():
    from ocvfacerec.facerec.feature import SpatialHistogram
    from ocvfacerec.facerec.lbp import VarLBP
    from ocvfacerec.facerec.serialization import dumps_model, loads_model
    op = VarLBP(radius=2, neighbors=6)
    assert (op.radius, op.neighbors, repr(op)) == (2, 6, "VarLBP (neighbors=6, radius=2)")
    assert VarLBP.__module__ == "ocvfacerec.facerec.lbp" and vars(VarLBP()) == {"_neighbors": 8, "_radius": 1}
    back = loads_model(dumps_model(SpatialHistogram(op, (2, 3))))
    assert type(back.lbp_operator) is VarLBP and vars(back.lbp_operator) == vars(op) and back.sz == (2, 3)


@pytest.mark.parametrize("P,hist,code,text", [(1, False, -2, b">= 2"), (1, True, -2, b">= 2"), (33, False, -2, b"[1, 32]"),
                                              (16, True, -2, b"<= 15"), (8, True, -1, b"count_bytes")])
def test_argument_checks_need_no_device(P, hist, code, text):
    from opencv_facerecognizer_amd import _lib
    lib = _lib.load()
    offs, w = np.zeros((P, 4), np.int32), np.ones((P, 4))
    geom = (P, offs.ctypes.data_as(_lib.c_vp), w.ctypes.data_as(_lib.c_vp), 1, 1, 3, 3)
    if hist:
        rc = lib.ofr_varlbp_hist(None, None, 1, 1, 13, 18, *geom, 2, 3, None, 3 if code == -1 else 1, None)
    else:
        rc = lib.ofr_varlbp_values(None, None, 1, 1, 13, 18, *geom, None)
    assert rc == code and text in lib.ofr_last_error()
    assert lib.ofr_hist_density_f32(None, None, 1, None, 2, 6, 256, None, 1540) == -1 and b"ld" in lib.ofr_last_error()
