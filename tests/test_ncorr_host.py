"""NormalizedCorrelation (reference distance.py:80-98) exists under the reference's name, carries its
metric id and survives the whitelisted model reader; its entry points validate before any device work."""
from opencv_facerecognizer_amd import _lib


def test_class_name_and_id():
    import ocvfacerec.facerec.distance as D
    m = D.NormalizedCorrelation()
    assert m.name == "NormalizedCorrelation" and repr(m) == "NormalizedCorrelation"
    assert type(m).__module__ == "ocvfacerec.facerec.distance" and m.__dict__ == {"_name": "NormalizedCorrelation"}
    assert m.metric_id == _lib.METRIC_NCORR == 7 and _lib.METRIC_NCORR in _lib.HIST_METRICS


def test_model_round_trips(tmp_path):
    from ocvfacerec.facerec.classifier import NearestNeighbor
    from ocvfacerec.facerec.distance import NormalizedCorrelation
    from ocvfacerec.facerec.serialization import load_model, save_model
    save_model(str(tmp_path / "m.pkl"), NearestNeighbor(NormalizedCorrelation(), k=2))
    nn = load_model(str(tmp_path / "m.pkl"))
    assert type(nn.dist_metric) is NormalizedCorrelation and nn.k == 2 and nn._metric() == _lib.METRIC_NCORR


def test_entry_points_validate_first():
    lib = _lib.load()
    assert lib.ofr_ncorr_workspace_bytes(70, 300, 16) >= 5 * 70 * 16 * 8 + (70 + 300) * 16
    assert lib.ofr_ncorr_knn(None, 9, None, 1, 16, None, 1, 16, 16, 1, 0, None, None, None, 0, None) == -1
    assert b"dtype" in lib.ofr_last_error()
    assert lib.ofr_ncorr_knn(None, 0, None, 1, 16, None, 1, 16, 16, 17, 0, None, None, None, 0, None) == -2
    assert lib.ofr_knn_deep(None, 8, None, 1, 16, 3, None, 1, 16, 3, 16, 1.0, 1, 0, None, None, None, 0) == -1
