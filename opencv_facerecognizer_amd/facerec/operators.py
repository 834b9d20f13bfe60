"""Feature combinators (reference ``src/ocvfacerec/facerec/operators.py``).

``ChainOperator`` (operators.py:58-81) is the glue Fisherfaces uses to chain
PCA into LDA (feature.py:222-224).  CombineOperator/CombineOperatorND
(operators.py:84-157) are not on the hot path and are out of scope.
"""
from __future__ import annotations

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


for _c in (FeatureOperator, ChainOperator):
    _c.__module__ = "ocvfacerec.facerec.operators"
