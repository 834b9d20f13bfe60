"""The float preprocessing entry points without a device: their argument checks come before any device work."""
import pytest

from opencv_facerecognizer_amd import _lib


def tt(pixel_bytes=4, alpha=0.1, tau=10.0, gamma=0.2, s0=1.0, s1=2.0):
    return _lib.load().ofr_tantriggs_f32_f(None, None, pixel_bytes, 1, 16, 16, alpha, tau, gamma, s0, s1, None, None, 0)


@pytest.mark.parametrize("bad, word", [({"alpha": 0.0}, b"alpha"), ({"tau": -1.0}, b"tau"), ({"s0": 0.0}, b"sigma"),
                                       ({"s1": 4.2}, b"radius"), ({"pixel_bytes": 2}, b"pixel_bytes"),
                                       ({"pixel_bytes": 8, "s1": 4.1}, b"null")])     # radius 16 is served
def test_tantriggs_argument_checks(bad, word):
    assert tt(**bad) == -1 and word in _lib.load().ofr_last_error()


@pytest.mark.parametrize("pixel_bytes, num_bins, word", [(4, 0, b"num_bins"), (8, 4097, b"num_bins"),
                                                         (2, 256, b"pixel_bytes"), (4, 256, b"null")])
def test_histeq_argument_checks(pixel_bytes, num_bins, word):
    lib = _lib.load()
    assert lib.ofr_histeq_f64_f(None, None, pixel_bytes, 1, 16, 16, num_bins, None) == -1
    assert word in lib.ofr_last_error()


def test_workspace_follows_the_float_strip_plane():
    lib = _lib.load()
    assert lib.ofr_tantriggs_workspace_bytes_f(4, 113, 113, 1.0, 2.0) == 0      # resident: no workspace
    assert lib.ofr_tantriggs_workspace_bytes_f(4, 114, 114, 1.0, 2.0) == 4 * 2 * 2 * 8   # strips of 112 + 2 rows
    assert lib.ofr_tantriggs_workspace_bytes(4, 114, 114, 1.0, 2.0) == 0        # the byte kernel's split differs
