"""PredictableModel (reference ``src/ocvfacerec/facerec/model.py:39-60``).

``compute``/``predict`` keep the reference contract; ``predict_batch`` is the
batched entry point of the device path.  Two fused pipelines, in which the
features never leave the GPU:
* Fisherfaces + NearestNeighbor (Euclidean/Cosine): a batch of faces is
  projected (exact int8-slice MFMA kernel, the gallery centring folded into the
  projection's shift) and searched by the certified tiers;
* LBPH, SpatialHistogram(ExtendedLBP, OriginalLBP or LPQ) + NearestNeighbor(
  ChiSquare, or HistogramIntersection / the BinRatio family) (feature.py:266-305,
  distance.py:101-183): ONE histogram launch per batch (``ofr_elbp_hist``,
  ``ofr_olbp_hist`` or ``ofr_lpq_hist``) gives the
  integer cell histograms, searched as counts against the counts gallery
  ``compute`` left on the device (``ofr_chi2_knn`` / ``ofr_hist_knn``).  The same with
  preprocessing chained in front (``ChainOperator``; TanTriggsPreprocessing, HistogramEqualization or
  a ChainOperator of them at any depth): one launch per preprocessing step, whose float faces go to
  the next step's float kernel and to the float histogram kernels (``ofr_*_hist_f``) on the device,
  then the counts search.  A ``VarLBP`` operator has one denominator per cell, so its route carries fp32
  rows instead of counts: ``ofr_varlbp_hist`` + ``ofr_hist_density_f32`` per batch, searched against the
  fp32 gallery ``compute`` left on the device.  A multi-scale LBP histogram,
  ``CombineOperator(SpatialHistogram(ExtendedLBP(r, P), sz), ...)`` of 2..4 scales (``operators.fused_scales``),
  bare or behind preprocessing, carries fp32 rows too: ONE ``ofr_mslbp_hist`` launch per batch gives the
  rows of all scales, searched against the fp32 gallery ``compute`` left on the device.  The route is chosen
  by the tree alone: faces of a size the kernel does not take (``fused_scales`` is None for it) still go this
  way, and ``CombineOperator.density_batch`` then builds their rows from the members' own kernels on the host
  and uploads them -- correct, but a host round trip per batch;
* ChainOperator(preprocessing as above, Fisherfaces) + NearestNeighbor (Euclidean/Cosine): the
  preprocessing launches (``ofr_tantriggs_f32`` / ``ofr_histeq_f64`` and their ``_f`` twins for
  float faces), one fp64 projection with the gallery centring folded in, one search.
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from .classifier import AbstractClassifier, NearestNeighbor, results
from .feature import AbstractFeature, Fisherfaces, SpatialHistogram
from .lbp import LPQ, ExtendedLBP, OriginalLBP, VarLBP
from .operators import ChainOperator, CombineOperator
from .preprocessing import HistogramEqualization, TanTriggsPreprocessing


def _preprocessing(f):
    """TanTriggsPreprocessing, HistogramEqualization, or a ChainOperator of them at any depth."""
    if type(f) is ChainOperator:
        return _preprocessing(f.model1) and _preprocessing(f.model2)
    return type(f) in (TanTriggsPreprocessing, HistogramEqualization)


def _preprocessed(f):
    """ChainOperator(preprocessing, feature): the device routes run model1's launches in front of model2."""
    return type(f) is ChainOperator and _preprocessing(f.model1)


def _size_groups(X):
    """Faces -> (X as a list or one-size batch, [(positions or None, faces of one size)])."""
    if hasattr(X, "device") or (isinstance(X, np.ndarray) and X.ndim == 3):   # one face size
        return X, [(None, X)]
    X = list(X)
    shapes = {}
    for i, x in enumerate(X):
        shapes.setdefault(np.asarray(x).shape, []).append(i)
    return X, [(sel, [X[i] for i in sel]) for sel in shapes.values()]


class PredictableModel(object):
    def __init__(self, feature, classifier):
        if not isinstance(feature, AbstractFeature):
            raise TypeError("feature must be of type AbstractFeature!")
        if not isinstance(classifier, AbstractClassifier):
            raise TypeError("classifier must be of type AbstractClassifier!")
        self.feature = feature
        self.classifier = classifier

    def compute(self, X, y):
        """model.py:49-51.  When the feature left its training features on the device, the classifier
        builds its device gallery from them (no host round trip of the gallery)."""
        features = self.feature.compute(X, y)
        self.classifier.compute(features, y)
        chained = self._lbph_chain() or (self._mslbp() and _preprocessed(self.feature))
        holder = self.feature.model2 if chained else self.feature   # who left device features
        dev = holder.__dict__.pop("_dev_features", None)
        if dev is None or dev[0] != id(features):
            return
        if isinstance(dev[1], tuple) and dev[1][0] == "counts":       # SpatialHistogram counts
            if hasattr(self.classifier, "adopt_device_counts"):
                _, C, cell, cb = dev[1]
                self.classifier.adopt_device_counts(C, cell, cb)
        elif isinstance(dev[1], tuple) and dev[1][0] == "hist":       # fp32 rows: VarLBP, multi-scale LBP
            if hasattr(self.classifier, "adopt_device_hist"):
                self.classifier.adopt_device_hist(dev[1][1], dev[1][2])
        elif hasattr(self.classifier, "adopt_device_rows"):
            self.classifier.adopt_device_rows(dev[1])

    def shard(self, group=None):
        """Shard the classifier's gallery over the ranks of ``group`` (NearestNeighbor.shard): every
        rank then predicts the same faces and gets the global result."""
        self.classifier.shard(group)
        return self

    def predict(self, X):
        """model.py:53-55 (one face)."""
        # one face: the reference's own order, extract then classify
        if self._chain() or self._lbph_chain() or self._varlbp() or self._mslbp():
            return self.classifier.predict(self.feature.extract(X))
        return self.predict_batch([X])[0]

    def search_batch(self, X, k=None):
        """Batch of faces -> (distances fp64 [B,k], gallery indices int64 [B,k]) host arrays."""
        d, i = self._search_device(X, k)
        return d.cpu().numpy(), i.cpu().numpy()

    def _fused(self):
        return (isinstance(self.feature, Fisherfaces) and type(self.classifier) is NearestNeighbor
                and getattr(self.classifier.dist_metric, "metric_id", None) in (0, 1))

    def _chain(self):
        f = self.feature
        return (_preprocessed(f)
                and isinstance(f.model2, Fisherfaces) and type(self.classifier) is NearestNeighbor
                and getattr(self.classifier.dist_metric, "metric_id", None) in (0, 1))

    def _lbph_chain(self):
        """ChainOperator(preprocessing, SpatialHistogram): the LBPH route with the preprocessing launches in
        front."""
        f = self.feature
        return (_preprocessed(f)
                and type(f.model2) is SpatialHistogram and self._lbph())

    def _lbph(self):
        f = self.feature
        if _preprocessed(f):
            f = f.model2
        return (type(f) is SpatialHistogram and isinstance(f.lbp_operator, (ExtendedLBP, OriginalLBP, LPQ, VarLBP))
                and type(self.classifier) is NearestNeighbor
                and getattr(self.classifier.dist_metric, "metric_id", None) in _lib.HIST_METRICS)

    def _varlbp(self):
        f = self.feature.model2 if _preprocessed(self.feature) else self.feature
        return self._lbph() and isinstance(f.lbp_operator, VarLBP)

    def _mslbp(self):
        """A multi-scale LBP histogram (a CombineOperator that takes device batches), bare or behind
        preprocessing, searched with a histogram metric."""
        f = self.feature.model2 if _preprocessed(self.feature) else self.feature
        return (type(f) is CombineOperator and f.device_batches and type(self.classifier) is NearestNeighbor
                and getattr(self.classifier.dist_metric, "metric_id", None) in _lib.HIST_METRICS)

    def _search_device(self, X, k=None):
        clf = self.classifier
        k = int(clf.k if k is None else k)
        if self._lbph():
            return self._search_lbph(X, k)
        if self._mslbp():
            return self._search_density(X, k)
        g = clf._gallery()
        proj = self.feature
        if self._chain():     # illumination normalisation on the device, its float faces go to the fp64 GEMM
            proj = self.feature.model2
            X = self.feature.model1.extract_batch(X)
        if g.N and g.d != proj._proj().d:
            raise ValueError("feature dimension does not match the classifier gallery")
        # Euclidean: the gallery centring is folded into the projection (W^T x - c, fp64, rounded once)
        Qd = proj.project_device(X, shift64=g.shift64)
        return clf._search_prepared(Qd, k)

    def _search_lbph(self, X, k):
        """LBPH batch: faces grouped by size, one histogram launch + one counts search per group (behind a
        preprocessing step: its launch first, the float faces stay on the device).  VarLBP: one histogram
        and one density launch per group, then one search of all the fp32 rows."""
        import torch
        if self._varlbp():
            return self._search_density(X, k)
        if self._lbph_chain():
            pre, sh = self.feature.model1, self.feature.model2

            def counts_batch(xs):
                return sh.counts_batch(pre.extract_batch(xs))
        else:
            counts_batch = self.feature.counts_batch
        X, groups = _size_groups(X)
        if len(groups) == 1:
            C, cell, cb = counts_batch(groups[0][1])
            return self.classifier.search_counts(C, cell, cb, k)
        # a group whose cell size differs from the counts gallery's comes back on the host
        # (search_counts' float path): every group's result goes to the gallery device
        B = len(X)
        dev = _lib.device()
        d_all = i_all = None
        for sel, xs in groups:
            C, cell, cb = counts_batch(xs)
            d, i = self.classifier.search_counts(C, cell, cb, k)
            if d_all is None:
                d_all = torch.empty((B,) + tuple(d.shape[1:]), dtype=d.dtype, device=dev)
                i_all = torch.empty((B,) + tuple(i.shape[1:]), dtype=i.dtype, device=dev)
            idx = torch.tensor(sel, dtype=torch.int64, device=dev)
            d_all.index_copy_(0, idx, d.to(dev, d_all.dtype))
            i_all.index_copy_(0, idx, i.to(dev, i_all.dtype))
        return d_all, i_all

    def _search_density(self, X, k):
        """VarLBP and multi-scale LBP: the preprocessing launches, one ``density_batch`` per face size, one search
        of all the fp32 rows."""
        import torch
        chained = _preprocessed(self.feature)
        sh = self.feature.model2 if chained else self.feature
        pre = self.feature.model1 if chained else None
        X, groups = _size_groups(X)
        rows = [sh.density_batch(pre.extract_batch(xs) if pre is not None else xs) for _, xs in groups]
        if len(groups) == 1:
            return self.classifier.search_density(rows[0], k)
        # every size gives rows of the same width (cells * 2^P): back into the callers' order, one search
        F = torch.empty((len(X), rows[0].shape[1]), dtype=rows[0].dtype, device=rows[0].device)
        for (sel, _), r in zip(groups, rows):
            F.index_copy_(0, torch.tensor(sel, dtype=torch.int64, device=F.device), r)
        return self.classifier.search_density(F, k)

    def predict_batch(self, X):
        """Predict a batch of faces (list of 2-D arrays, an array [B, H, W], or a uint8 device
        tensor [B, H, W] such as ``ingest.faces`` returns)."""
        if not (self._fused() or self._lbph() or self._chain() or self._mslbp()):
            if hasattr(X, "data_ptr"):   # a device face batch: the generic path works on host items
                X = list(X.cpu().numpy())
            qs = [self.feature.extract(x) for x in X]
            return self.classifier.predict_batch(qs) if hasattr(self.classifier, "predict_batch") else \
                [self.classifier.predict(q) for q in qs]
        if len(X) == 0:
            return []
        d_all, i_all = self.search_batch(X)
        return results(d_all, i_all, self.classifier.y)

    def __repr__(self):
        feature_repr = repr(self.feature)
        classifier_repr = repr(self.classifier)
        return "PredictableModel (feature=%s, classifier=%s)" % (feature_repr, classifier_repr)


PredictableModel.__module__ = "ocvfacerec.facerec.model"
