"""Local binary patterns (reference ``src/ocvfacerec/facerec/lbp.py``).

``ExtendedLBP`` (lbp.py:75-137) keeps its interface (``__call__(X)`` ->
uint32 code image, ``neighbors``, ``radius``) and pickled state
(``_neighbors``, ``_radius``).  The sampling geometry is derived on the host
exactly as the reference derives it (np.sin/np.cos, lbp.py:84-121); the codes
are computed by the ``ofr_elbp_codes`` kernel, which reproduces the
reference's float64 interpolation order bit for bit (see ofr_lbp.hip).

``OriginalLBP`` (lbp.py:55-72) and ``LPQ`` (lbp.py:211-318) keep their
constructor arguments, ``repr`` and pickled state; their 8-bit codes come from
``ofr_olbp_codes`` / ``ofr_lpq_codes`` (ofr_lpq.hip).  OriginalLBP is
bit-exact.  LPQ runs in fp64 with the decorrelation matrix ``V`` derived on
the host (``LPQ.basis``) and agrees with the reference wherever the
decorrelated responses are above rounding noise (on a window of
constant grey every response is zero up to noise and the reference's own code
is the sign of that noise).

Images.  8-bit grey images -- uint8, or any array whose values are integers in
0..255 -- take the byte kernels.  2-D float32 / float64 images of arbitrary
values (what ``TanTriggsPreprocessing`` and ``HistogramEqualization`` return)
take the float kernels (``ofr_*_f``, ofr_lbp_float.hip): every pixel is
converted exactly to float64 and all arithmetic is float64, which is what the
installed numpy 2.x does with the reference on a float image.  One quirk of the
reference is kept, not fixed: ExtendedLBP's centre is
``np.asarray(X[...], dtype=np.uint8)`` (lbp.py:104), i.e.
``C = trunc(x).astype(int64) & 255`` -- floor for 0 <= x < 256 and wrap-around
outside it (-3.7 -> 253, 300.7 -> 44), so the negative half of a Tan-Triggs face
has centres near 255.  OriginalLBP compares the values as given.  Codes touching
a non-finite pixel (a constant face under Tan-Triggs is 0/0) are unspecified;
they stay inside the histogram range.

``VarLBP`` (lbp.py:140-208) keeps its constructor, ``repr`` and pickled state
too.  ``__call__`` returns the float64 variance image of the ``ofr_varlbp_values``
kernel (ofr_varlbp.hip): ExtendedLBP's geometry, the reference's Welford
recurrence over the circle in float64 with IEEE divisions, bit for bit.  Its
values are real variances and many fall outside the histogram range, so under
``SpatialHistogram`` every cell has its own denominator.
"""
from __future__ import annotations

import numpy as np


class LocalDescriptor(object):
    """lbp.py:40-52."""

    def __init__(self, neighbors):
        self._neighbors = neighbors

    def __call__(self, X):
        raise NotImplementedError("Every LBPOperator must implement the __call__ method.")

    @property
    def neighbors(self):
        return self._neighbors

    def __repr__(self):
        return "LBPOperator (neighbors=%s)" % (self._neighbors)


def elbp_geometry(radius, neighbors):
    """lbp.py:84-121: ((oy, ox), (by, bx), offsets int32 [P,4] = (fy, fx, cy, cx), weights fp64 [P,4])."""
    angles = 2 * np.pi / neighbors
    theta = np.arange(0, 2 * np.pi, angles)
    sample_points = np.array([-np.sin(theta), np.cos(theta)]).T
    sample_points *= radius
    miny = min(sample_points[:, 0])
    maxy = max(sample_points[:, 0])
    minx = min(sample_points[:, 1])
    maxx = max(sample_points[:, 1])
    blocksizey = np.ceil(max(maxy, 0)) - np.floor(min(miny, 0)) + 1
    blocksizex = np.ceil(max(maxx, 0)) - np.floor(min(minx, 0)) + 1
    origy = 0 - np.floor(min(miny, 0))
    origx = 0 - np.floor(min(minx, 0))
    offs = np.zeros((len(sample_points), 4), np.int32)
    wts = np.zeros((len(sample_points), 4), np.float64)
    for i, p in enumerate(sample_points):
        y, x = p + (origy, origx)
        fx, fy = np.floor(x), np.floor(y)
        cx, cy = np.ceil(x), np.ceil(y)
        ty, tx = y - fy, x - fx
        wts[i] = ((1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty)
        offs[i] = (fy, fx, cy, cx)
    return (int(origy), int(origx)), (int(blocksizey), int(blocksizex)), offs, wts


def as_u8_images(X):
    """Image or stack of images -> uint8 array; values must already be integers in [0, 255]."""
    X = np.asanyarray(X)
    if X.dtype == np.uint8:
        return X
    if X.dtype.kind in "iub" or X.dtype.kind == "f":
        Xi = X.astype(np.uint8)
        if np.array_equal(Xi.astype(X.dtype), X):
            return Xi
    raise NotImplementedError("the LBP operators (MI355X build) accept 8-bit grey images (integer values 0..255)")


def as_pixel_images(X):
    """Image or stack of images -> what the kernels take: uint8 where ``as_u8_images`` gives it (the byte
    kernels), float32 / float64 arrays of any other values as they are (the float kernels)."""
    X = np.asanyarray(X)
    if X.dtype in (np.float32, np.float64):
        with np.errstate(invalid="ignore"):     # NaN / out-of-range values: not integer-valued
            Xi = X.astype(np.uint8)
            return Xi if np.array_equal(Xi.astype(X.dtype), X) else np.asarray(X)
    return as_u8_images(X)


def _device_image(X, who):
    """One 2-D image -> device stack [1][H][W] of its kernel dtype."""
    from .. import _device
    X = as_pixel_images(X)
    if X.ndim != 2:
        raise ValueError("%s expects a 2-D image" % who)
    return _device.pixel_images(X[None])


class ExtendedLBP(LocalDescriptor):
    """lbp.py:75-137 on the GPU."""

    def __init__(self, radius=1, neighbors=8):
        LocalDescriptor.__init__(self, neighbors=neighbors)
        self._radius = radius

    def geometry(self):
        return elbp_geometry(self._radius, self._neighbors)

    def __call__(self, X):
        from .. import _device
        codes = _device.elbp_codes(_device_image(X, "ExtendedLBP"), self.geometry())
        return codes.cpu().numpy()[0].view(np.uint32)

    def codes_batch(self, imgs_u8_device):
        """uint8, float32 or float64 [n][H][W] device tensor -> int32-stored uint32 codes [n][dy][dx] (device)."""
        from .. import _device
        return _device.elbp_codes(_device.pixel_images(imgs_u8_device), self.geometry())

    @property
    def radius(self):
        return self._radius

    def __repr__(self):
        return "ExtendedLBP (neighbors=%s, radius=%s)" % (self._neighbors, self._radius)


class VarLBP(LocalDescriptor):
    """lbp.py:140-208 on the GPU: the variance of the circle's samples, float64 [dy][dx]."""

    def __init__(self, radius=1, neighbors=8):
        LocalDescriptor.__init__(self, neighbors=neighbors)
        self._radius = radius

    def geometry(self):
        return elbp_geometry(self._radius, self._neighbors)

    def __call__(self, X):
        from .. import _device
        return _device.varlbp_values(_device_image(X, "VarLBP"), self.geometry()).cpu().numpy()[0]

    def values_batch(self, imgs_device):
        """uint8, float32 or float64 [n][H][W] device tensor -> float64 variances [n][dy][dx] (device)."""
        from .. import _device
        return _device.varlbp_values(_device.pixel_images(imgs_device), self.geometry())

    @property
    def radius(self):
        return self._radius

    def __repr__(self):
        return "VarLBP (neighbors=%s, radius=%s)" % (self._neighbors, self._radius)


class OriginalLBP(LocalDescriptor):
    """lbp.py:55-72 on the GPU: the 3x3 operator, codes [H-2][W-2]."""

    def __init__(self):
        LocalDescriptor.__init__(self, neighbors=8)

    def __call__(self, X):
        from .. import _device
        return _device.olbp_codes(_device_image(X, "OriginalLBP")).cpu().numpy()[0].astype(np.int64)

    def __repr__(self):
        return "OriginalLBP (neighbors=%s)" % (self._neighbors)


_LPQ_BASIS = {}


def lpq_basis(radius):
    """lbp.py:244-276: the 8x8 matrix ``np.linalg.svd(D)`` returns third (the kernel applies its transpose).
    Derived, not tabulated: the two largest singular values of D are equal, so the basis inside their
    plane belongs to the host's LAPACK.  Cached per radius."""
    if radius not in _LPQ_BASIS:
        f = 1.0
        x = np.arange(-radius, radius + 1)
        n = len(x)
        rho = 0.95
        [xp, yp] = np.meshgrid(np.arange(1, (n + 1)), np.arange(1, (n + 1)))
        pp = np.concatenate((xp, yp)).reshape(2, -1)
        dd = _euc_dist(pp.T)
        C = np.power(rho, dd)
        w0 = (x * 0.0 + 1.0)
        w1 = np.exp(-2 * np.pi * 1j * x * f / n)
        w2 = np.conj(w1)
        q1 = w0.reshape(-1, 1) * w1
        q2 = w1.reshape(-1, 1) * w0
        q3 = w1.reshape(-1, 1) * w1
        q4 = w1.reshape(-1, 1) * w2
        M = np.array([u.flatten('F') for q in (q1, q2, q3, q4) for u in (np.real(q), np.imag(q))])
        D = np.dot(np.dot(M, C), M.T)
        U, S, V = np.linalg.svd(D)
        _LPQ_BASIS[radius] = np.ascontiguousarray(V, dtype=np.float64)
    return _LPQ_BASIS[radius]


def _euc_dist(X):
    """lbp.py:231-241."""
    Y = X = X.astype(float)
    XX = np.sum(X * X, axis=1)[:, np.newaxis]
    YY = XX.T
    distances = np.dot(X, Y.T)
    distances *= -2
    distances += XX
    distances += YY
    np.maximum(distances, 0, distances)
    distances.flat[::distances.shape[0] + 1] = 0.0
    return np.sqrt(distances)


class LPQ(LocalDescriptor):
    """lbp.py:211-318 on the GPU: local phase quantization, codes [H][W] in the reference's order (the
    code of pixel (r, c) sits at linear index c*H + r)."""

    def __init__(self, radius=3):
        LocalDescriptor.__init__(self, neighbors=8)
        self._radius = radius

    def euc_dist(self, X):
        return _euc_dist(X)

    def basis(self):
        return lpq_basis(int(self._radius))

    def __call__(self, X):
        from .. import _device
        codes = _device.lpq_codes(_device_image(X, "LPQ"), int(self._radius), self.basis())
        return codes.cpu().numpy()[0].astype(np.int64)

    @property
    def radius(self):
        return self._radius

    def __repr__(self):
        return "LPQ (neighbors=%s, radius=%s)" % (self._neighbors, self._radius)


for _c in (LocalDescriptor, ExtendedLBP, VarLBP, OriginalLBP, LPQ):
    _c.__module__ = "ocvfacerec.facerec.lbp"
