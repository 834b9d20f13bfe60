"""HistogramIntersection and the BinRatio family (reference distance.py:119-183) exist under the
reference's names, survive the whitelisted model reader, and their ids and entry points are bound."""
import pytest

from opencv_facerecognizer_amd import _lib

CLASSES = [("HistogramIntersection", "HistogramIntersection", 3), ("BinRatioDistance", "BinRatioDistance", 4),
           ("L1BinRatioDistance", "L1-BinRatioDistance", 5), ("ChiSquareBRD", "ChiSquare-BinRatioDistance", 6)]


@pytest.mark.parametrize("cls,name,mid", CLASSES)
def test_class_names_and_ids(cls, name, mid):
    import ocvfacerec.facerec.distance as D
    m = getattr(D, cls)()
    assert m.name == name and repr(m) == name
    assert type(m).__module__ == "ocvfacerec.facerec.distance"
    assert m.metric_id == mid and mid in _lib.HIST_METRICS


def test_model_with_a_histogram_metric_round_trips():
    from ocvfacerec.facerec.classifier import NearestNeighbor
    from ocvfacerec.facerec.distance import HistogramIntersection
    from ocvfacerec.facerec.serialization import dumps_model, loads_model
    nn = loads_model(dumps_model(NearestNeighbor(HistogramIntersection(), k=2)))
    assert type(nn.dist_metric) is HistogramIntersection and nn.k == 2


def test_lib_exposes_ids_and_symbols():
    assert (_lib.METRIC_HISTINTERSECT, _lib.METRIC_BINRATIO, _lib.METRIC_L1BINRATIO, _lib.METRIC_CHISQBRD) == (3, 4, 5, 6)
    lib = _lib.load()
    assert lib.ofr_hist_workspace_bytes(70, 300, 16) >= 5 * 70 * 16 * 8
    # argument validation precedes any device work
    assert lib.ofr_hist_knn(None, 2, 0, None, 1, 16, None, 1, 16, 16, 1.0, 1, 0, None, None, None, 0, None) == -1
    assert b"metric" in lib.ofr_last_error()
    assert lib.ofr_hist_knn(None, 3, 0, None, 1, 16, None, 1, 16, 16, 1.0, 17, 0, None, None, None, 0, None) == -2
