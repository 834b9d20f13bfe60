"""Illumination normalisation (reference ``src/ocvfacerec/facerec/preprocessing.py``).

``TanTriggsPreprocessing`` (preprocessing.py:83-109) and ``HistogramEqualization``
(preprocessing.py:62-80) keep their constructor arguments, ``repr`` and pickled
state (``_alpha``, ``_tau``, ``_gamma``, ``_sigma0``, ``_sigma1`` / ``_num_bins``).
Their arithmetic runs in ``ofr_tantriggs_f32`` / ``ofr_histeq_f64``
(ofr_preproc.hip, 8-bit faces) and ``ofr_tantriggs_f32_f`` / ``ofr_histeq_f64_f``
(ofr_preproc_float.hip, float32 / float64 faces): ``compute`` makes one launch per
group of same-sized faces, ``extract`` handles one face, and ``extract_batch`` (new)
takes a list, an array ``[n][H][W]`` or a uint8 / float32 / float64 device tensor and
leaves the result on the device, where the other preprocessing step,
``Fisherfaces.project_device`` (``ChainOperator.extract_batch``,
``PredictableModel.predict_batch``), ``SpatialHistogram.counts_batch`` and ``compute``
(the LBPH route; the LBP kernels take float faces) consume it.  Host input goes
through ``lbp.as_pixel_images``: integer-valued faces of any dtype keep the byte
kernels, any other float32 / float64 face takes the float kernels -- so
``ChainOperator(TanTriggsPreprocessing(), HistogramEqualization())`` (and the other
order) works as in the reference, on the device from end to end.  Any other device
dtype is a ``TypeError``.

Tan-Triggs returns float32 like the reference; its filter accumulates in fp64,
so it sits closer to the exact result than the reference's own float32 run
(DESIGN.md).  A constant face is 0/0 in the reference (rounding noise or NaN
there): here the values are unspecified too, and nothing traps.
``HistogramEqualization`` follows the installed numpy, where the reference's
``normed=True`` is spelled ``density=True``, bin for bin.

``LBPPreprocessing`` (preprocessing.py:112-127) is a thin class over the LBP
code kernels of ``lbp.py``.

Out of scope: ``Resize`` (preprocessing.py:44-59; ``scipy.misc.imresize`` no
longer exists, ``ingest.faces`` is this package's resize) and
``MinMaxNormalizePreprocessing`` / ``ZScoreNormalizePreprocessing``
(preprocessing.py:130-171; elementwise on arbitrary features, no hot path).
"""
from __future__ import annotations

import numpy as np
import torch

from .feature import AbstractFeature
from .lbp import ExtendedLBP, as_pixel_images


class _DevicePreprocessing(AbstractFeature):
    """Batch plumbing shared by the kernels; a subclass supplies ``_run(device [n][H][W])`` for uint8,
    float32 and float64 pixels."""

    device_batches = True     # compute takes a device face batch (ChainOperator.compute)

    def _run(self, imgs):
        raise NotImplementedError

    def extract_batch(self, X):
        """Faces of one size (list, array [n][H][W] or a uint8 / float32 / float64 device tensor [n][H][W],
        e.g. from ``ingest.faces`` or from another preprocessing step) -> device tensor [n][H][W], one
        launch."""
        from .. import _device
        if hasattr(X, "data_ptr"):
            if X.dtype not in (torch.uint8, torch.float32, torch.float64):
                raise TypeError("device face batches must be uint8, float32 or float64")
            return self._run(X)
        if not (isinstance(X, np.ndarray) and X.ndim == 3):
            X = np.stack([np.asarray(x) for x in X])
        return self._run(_device.pixel_images(as_pixel_images(X)))

    def compute_device(self, X, y):
        """``compute`` for a consumer on the device (``ChainOperator.compute``): faces of one size -> device
        tensor [n][H][W], one launch; None for mixed sizes or no faces (the caller takes ``compute``)."""
        if hasattr(X, "data_ptr") or (isinstance(X, np.ndarray) and X.ndim == 3):
            return self.extract_batch(X) if len(X) else None
        X = [np.asarray(x) for x in X]
        if not X or any(x.shape != X[0].shape for x in X):
            return None
        return self.extract_batch(X)

    def compute(self, X, y):
        if hasattr(X, "data_ptr"):
            return list(self.extract_batch(X).cpu().numpy())
        X = [np.asarray(x) for x in X]
        out = [None] * len(X)
        shapes = {}
        for i, x in enumerate(X):
            shapes.setdefault(x.shape, []).append(i)
        for sel in shapes.values():   # faces of one size per launch
            res = self.extract_batch([X[i] for i in sel]).cpu().numpy()
            for j, i in enumerate(sel):
                out[i] = res[j]
        return out

    def extract(self, X):
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError("%s expects a 2-D image" % type(self).__name__)
        return self.extract_batch(X[None]).cpu().numpy()[0]


class HistogramEqualization(_DevicePreprocessing):
    """preprocessing.py:62-80 on the GPU: float64 images in 0..255."""

    def __init__(self, num_bins=256):
        AbstractFeature.__init__(self)
        self._num_bins = num_bins

    def _run(self, imgs):
        from .. import _device
        return _device.histeq(imgs, int(self._num_bins))

    def __repr__(self):
        return "HistogramEqualization (num_bins=%s)" % (self._num_bins)


class TanTriggsPreprocessing(_DevicePreprocessing):
    """preprocessing.py:83-109 on the GPU: float32 images."""

    def __init__(self, alpha=0.1, tau=10.0, gamma=0.2, sigma0=1.0, sigma1=2.0):
        AbstractFeature.__init__(self)
        self._alpha = float(alpha)
        self._tau = float(tau)
        self._gamma = float(gamma)
        self._sigma0 = float(sigma0)
        self._sigma1 = float(sigma1)

    def _run(self, imgs):
        from .. import _device
        return _device.tantriggs(imgs, self._alpha, self._tau, self._gamma, self._sigma0, self._sigma1)

    def __repr__(self):
        return "TanTriggsPreprocessing (alpha=%.3f,tau=%.3f,gamma=%.3f,sigma0=%.3f,sigma1=%.3f)" % (
            self._alpha, self._tau, self._gamma, self._sigma0, self._sigma1)


class LBPPreprocessing(AbstractFeature):
    """preprocessing.py:112-127: the LBP code image of each face.  The operators take float images
    (lbp.py), so this class also works behind ``TanTriggsPreprocessing`` / ``HistogramEqualization`` in a
    ``ChainOperator``, with no code of its own for that."""

    def __init__(self, lbp_operator=ExtendedLBP(radius=1, neighbors=8)):
        AbstractFeature.__init__(self)
        self._lbp_operator = lbp_operator

    def compute(self, X, y):
        return [self.extract(xi) for xi in X]

    def extract(self, X):
        return self._lbp_operator(X)

    def __repr__(self):
        return "LBPPreprocessing (lbp_operator=%s)" % (repr(self._lbp_operator))


for _c in (_DevicePreprocessing, HistogramEqualization, TanTriggsPreprocessing, LBPPreprocessing):
    _c.__module__ = "ocvfacerec.facerec.preprocessing"
