"""Feature combinators (reference ``src/ocvfacerec/facerec/operators.py``).

``ChainOperator`` (operators.py:58-81) is the glue Fisherfaces uses to chain
PCA into LDA (feature.py:222-224).

``CombineOperator`` / ``CombineOperatorND`` (operators.py:84-157) concatenate the
features of two models; any pair of members works through the members' own
``compute`` / ``extract`` (each member runs its own device kernels).  One
combination has a kernel of its own, the multi-scale LBP histogram

    CombineOperator(SpatialHistogram(ExtendedLBP(1, 8), sz), SpatialHistogram(ExtendedLBP(2, 8), sz))

nested once or twice more for further radii: when ``fused_scales`` holds, all
scales of a batch of same-sized faces come out of ONE ``ofr_mslbp_hist`` launch
(ofr_mslbp.hip), as integer counts (the float64 features are counts / cell,
exactly) and / or as the fp32 rows the histogram searches take.
"""
from __future__ import annotations

import numpy as np

from .feature import AbstractFeature


class FeatureOperator(AbstractFeature):
    """operators.py:39-55."""

    def __init__(self, model1, model2):
        if (not isinstance(model1, AbstractFeature)) or (not isinstance(model2, AbstractFeature)):
            raise Exception("A FeatureOperator only works on classes implementing an AbstractFeature!")
        self.model1 = model1
        self.model2 = model2

    def __repr__(self):
        return "FeatureOperator(" + repr(self.model1) + "," + repr(self.model2) + ")"


class ChainOperator(FeatureOperator):
    """operators.py:58-81: model2.compute(model1.compute(X, y), y).  A model1 with ``compute_device`` (the
    preprocessing kernels) in front of a model2 that takes device batches (``device_batches``:
    SpatialHistogram, the preprocessing steps) keeps training faces of one size on the device between the
    two.  A chain offers the same two hooks itself -- ``compute_device`` when both members have it,
    ``device_batches`` when model2 has it -- so a nested chain of preprocessing steps stays on the device."""

    def __init__(self, model1, model2):
        FeatureOperator.__init__(self, model1, model2)

    @property
    def compute_device(self):
        dev1 = getattr(self.model1, "compute_device", None)
        dev2 = getattr(self.model2, "compute_device", None)
        if dev1 is None or dev2 is None:
            raise AttributeError("compute_device")

        def run(X, y):
            Xd = dev1(X, y)
            return None if Xd is None else dev2(Xd, y)
        return run

    @property
    def device_batches(self):
        return getattr(self.model2, "device_batches", False)

    def compute(self, X, y):
        dev1 = getattr(self.model1, "compute_device", None)
        if dev1 is not None and getattr(self.model2, "device_batches", False):
            Xd = dev1(X, y)
            if Xd is not None:
                return self.model2.compute(Xd, y)
        X = self.model1.compute(X, y)
        return self.model2.compute(X, y)

    def extract(self, X):
        X = self.model1.extract(X)
        return self.model2.extract(X)

    def extract_batch(self, X):
        """Batch of extract: model1's ``extract_batch`` where it has one, and its device result goes
        straight to model2's ``project_device`` (fp64 device rows [B][d]) or ``extract_batch``."""
        batch1 = getattr(self.model1, "extract_batch", None)
        X = batch1(X) if batch1 is not None else [self.model1.extract(x) for x in X]
        if hasattr(self.model2, "project_device"):
            return self.model2.project_device(X, f64=True)
        if hasattr(self.model2, "extract_batch"):
            return self.model2.extract_batch(X)
        return [self.model2.extract(x) for x in (X.cpu().numpy() if hasattr(X, "data_ptr") else X)]

    def __repr__(self):
        return "ChainOperator(" + repr(self.model1) + "," + repr(self.model2) + ")"


_LDS_BYTES = 160 * 1024      # one gfx950 workgroup


def _scale_leaves(op):
    """The leaves of a CombineOperator tree, left to right, when they are 2..4
    SpatialHistogram(ExtendedLBP(r, P), sz) of one P in 2..8 and one grid; else None.  No face size yet."""
    from .feature import SpatialHistogram
    from .lbp import ExtendedLBP
    leaves, todo = [], [op]
    while todo:
        f = todo.pop()
        if type(f) is CombineOperator:
            todo += [f.model2, f.model1]
        else:
            leaves.append(f)
    if not (type(op) is CombineOperator and 2 <= len(leaves) <= 4):
        return None
    if not all(type(f) is SpatialHistogram and type(f.lbp_operator) is ExtendedLBP for f in leaves):
        return None
    P, sz = leaves[0].lbp_operator.neighbors, tuple(leaves[0].sz)
    if not (isinstance(P, (int, np.integer)) and 2 <= P <= 8 and len(sz) == 2 and min(sz) >= 1):
        return None
    if any(f.lbp_operator.neighbors != P or tuple(f.sz) != sz for f in leaves):
        return None
    return leaves


def fused_scales(op, H, W, pixel_bytes=8):
    """The scales of the fused multi-scale LBP route (``ofr_mslbp_hist``), left to right, for faces of H x W
    pixels of ``pixel_bytes`` (1: uint8; float32 and float64 faces are staged as 8-byte float64, the default) --
    or None when ``op`` takes the plain path: a tree of other members, mixed neighbours or grids, more than
    four scales, a scale whose cell holds no or more than 65535 code pixels, or one cell row of all scales
    (two bins per 32-bit counter + the pixel rows it touches) above a workgroup's 160 KiB of LDS.  Needs no
    device."""
    leaves = _scale_leaves(op)
    if leaves is None:
        return None
    gr, gc = leaves[0].sz
    py, halo = [], []
    for f in leaves:
        _, (by, bx), _, _ = f.lbp_operator.geometry()
        dy, dx = H - by + 1, W - bx + 1
        if dy < gr or dx < gc or (dy // gr) * (dx // gc) > 65535:
            return None
        py.append(dy // gr)
        halo.append(by - 1)
    words = len(leaves) * gc * (1 << leaves[0].lbp_operator.neighbors) // 2
    px_rows = max(max((r + 1) * p + h for p, h in zip(py, halo)) - r * min(py) for r in range(gr))
    plane = px_rows * W * (1 if pixel_bytes == 1 else 8)
    if -(-words // 4) * 16 + (-(-plane // 16) * 16 + 16 if pixel_bytes == 1 else plane) > _LDS_BYTES:
        return None
    return leaves


class CombineOperator(FeatureOperator):
    """operators.py:84-118: hstack of the two members' features, each reshaped (1, -1).

    A multi-scale LBP histogram tree (``fused_scales``) takes device batches (``device_batches``):
    ``counts_device`` / ``density_batch`` make one ``ofr_mslbp_hist`` launch per batch of same-sized faces,
    ``compute`` groups the faces by size, forms the float64 features exactly as counts / (py_s * px_s) and, for
    one face size, leaves the fp32 rows for the classifier's device gallery.  Everything else -- other
    members, or a face size the kernel does not take -- runs the members' own ``compute`` / ``extract``."""

    def __init__(self, model1, model2):
        FeatureOperator.__init__(self, model1, model2)

    @property
    def device_batches(self):
        return _scale_leaves(self) is not None

    def _launch(self, X, counts, rows):
        """Faces of one size -> what ``_device.mslbp_hist`` returns, or None when this size is not fused."""
        from .. import _device
        from .lbp import as_pixel_images
        if not hasattr(X, "data_ptr"):     # host faces (a numpy array has a .device too: ask for a tensor)
            X = as_pixel_images(np.ascontiguousarray(X) if isinstance(X, np.ndarray) and X.ndim == 3
                                else np.stack([np.asarray(x) for x in X]))
        imgs = _device.pixel_images(X)
        leaves = fused_scales(self, int(imgs.shape[1]), int(imgs.shape[2]), imgs.element_size())
        if leaves is None:
            return None
        return _device.mslbp_hist(imgs, [f.lbp_operator.geometry() for f in leaves], tuple(leaves[0].sz), counts, rows)

    def counts_device(self, X):
        """Faces of one size (list, array [n][H][W] or a uint8 / float32 / float64 device tensor) -> (uint16
        counts as an int16 device tensor [n][S][cells][2^P], [cell pixel count of every scale]), one launch."""
        out = self._launch(X, True, False)
        if out is None:
            raise NotImplementedError("counts_device serves the fused multi-scale LBP route (fused_scales)")
        return out[0], out[2]

    def density_batch(self, X):
        """Faces of one size (as ``counts_device`` takes them) -> fp32 device rows [n][S * cells * 2^P] of the
        features, each value (float)(count / cell): one launch.  A face size that is not fused gives the same
        rows from the members' own kernels, rounded on the host."""
        import torch
        out = self._launch(X, False, True)
        if out is not None:
            return out[1]
        from .. import _lib
        X = list(X.cpu().numpy()) if hasattr(X, "data_ptr") else list(X)
        rows = np.concatenate(self._combine(X, None)).astype(np.float32)
        return torch.from_numpy(rows).to(_lib.device())

    def _combine(self, X, y, extract=False):
        if extract:
            A, B = [self.model1.extract(X)], [self.model2.extract(X)]
        else:
            A, B = self.model1.compute(X, y), self.model2.compute(X, y)
        return [np.hstack((np.asarray(a).reshape(1, -1), np.asarray(b).reshape(1, -1))) for a, b in zip(A, B)]

    def _fused_features(self, X, keep_device=False):
        """X (list of faces, or a device batch) -> (list of float64 (1, N) features, device rows or None); None
        when some face size is not fused."""
        from .. import _device
        on_device = hasattr(X, "data_ptr")
        shapes = {}
        for i in ([] if on_device else range(len(X))):
            shapes.setdefault(np.asarray(X[i]).shape, []).append(i)
        groups = [(list(range(len(X))), X)] if on_device else [(sel, [X[i] for i in sel]) for sel in shapes.values()]
        out, dev = [None] * len(X), None
        for sel, xs in groups:     # faces of one size per launch
            rows = keep_device and len(groups) == 1
            res = self._launch(xs, True, rows)
            if res is None:
                return None, None
            C, R, cells = res
            c = _device.counts_numpy(C, 2).astype(np.float64)               # [n][S][cells][2^P]
            h = (c / np.asarray(cells, np.float64)[None, :, None, None]).reshape(len(sel), 1, -1)
            for j, i in enumerate(sel):
                out[i] = h[j]
            if rows:
                dev = ("hist", R, int(h.shape[2]))
        return out, dev

    def compute(self, X, y):
        if self.device_batches and len(X):
            feats, dev = self._fused_features(X, keep_device=True)
            if feats is not None:
                if dev is not None:      # one face size: the fp32 rows go to the classifier's device gallery
                    self.__dict__["_dev_features"] = (id(feats), dev)
                return feats
        if hasattr(X, "data_ptr"):       # a device batch of a chain in front: the members take host faces
            X = list(X.cpu().numpy())
        return self._combine(X, y)

    def extract(self, X):
        if self.device_batches:
            feats, _ = self._fused_features([X])
            if feats is not None:
                return feats[0]
        return self._combine(X, None, extract=True)[0]

    def __getstate__(self):
        st = dict(self.__dict__)
        st.pop("_dev_features", None)      # derived device state, never pickled
        return st

    def __repr__(self):
        return "CombineOperator(" + repr(self.model1) + "," + repr(self.model2) + ")"


class CombineOperatorND(FeatureOperator):
    """operators.py:121-157: the members' outputs stacked with np.hstack (np.vstack for hstack=False)."""

    def __init__(self, model1, model2, hstack=True):
        FeatureOperator.__init__(self, model1, model2)
        self._hstack = hstack

    def compute(self, X, y):
        A = self.model1.compute(X, y)
        B = self.model2.compute(X, y)
        stack = np.hstack if self._hstack else np.vstack
        return [stack((a, b)) for a, b in zip(A, B)]

    def extract(self, X):
        stack = np.hstack if self._hstack else np.vstack
        return stack((self.model1.extract(X), self.model2.extract(X)))

    def __repr__(self):
        return "CombineOperatorND(" + repr(self.model1) + "," + repr(self.model2) + ", hstack=" + str(
            self._hstack) + ")"


for _c in (FeatureOperator, ChainOperator, CombineOperator, CombineOperatorND):
    _c.__module__ = "ocvfacerec.facerec.operators"
