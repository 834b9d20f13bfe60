"""CombineOperator / CombineOperatorND host semantics and the fused-route predicate (no device needed)."""
import numpy as np
import pytest


def test_combine_operators_host():
    from ocvfacerec.facerec.feature import Identity, SpatialHistogram
    from ocvfacerec.facerec.lbp import ExtendedLBP, OriginalLBP
    from ocvfacerec.facerec.operators import CombineOperator, CombineOperatorND, fused_scales

    def sh(r, P=8, grid=(8, 8)):
        return SpatialHistogram(ExtendedLBP(r, P), grid)
    both = CombineOperator(CombineOperator(sh(3), sh(1)), CombineOperator(sh(2), sh(4)))
    assert [f.lbp_operator.radius for f in fused_scales(both, 128, 128)] == [3, 1, 2, 4]
    assert len(fused_scales(CombineOperator(sh(1), CombineOperator(sh(2), sh(2))), 128, 128, pixel_bytes=1)) == 3
    for op, (H, W) in [(CombineOperator(sh(1), sh(2, 6)), (128, 128)),            # mixed neighbours
                       (CombineOperator(sh(1), sh(2, 8, (4, 4))), (128, 128)),    # different grids
                       (CombineOperator(both, sh(1)), (128, 128)),                # five leaves
                       (CombineOperator(sh(1, 8, (1, 1)), sh(2, 8, (1, 1))), (260, 260)),   # 66564-pixel cell
                       (CombineOperator(sh(1), SpatialHistogram(OriginalLBP(), (8, 8))), (128, 128)),
                       (CombineOperator(sh(1), sh(2)), (11, 128)),                # radius 2: 7 code rows for 8 cell rows
                       (CombineOperator(sh(1, 8, (1, 64)), sh(2, 8, (1, 64))), (128, 4000)),   # one cell row above LDS
                       (sh(1), (128, 128))]:
        assert fused_scales(op, H, W) is None
    with pytest.raises(Exception, match="A FeatureOperator only works on classes implementing an AbstractFeature!"):
        CombineOperator(Identity(), "x")
    with pytest.raises(Exception, match="A FeatureOperator only works"):
        CombineOperatorND("x", Identity())
    assert repr(CombineOperator(Identity(), Identity())) == "CombineOperator(Identity,Identity)"
    assert repr(CombineOperatorND(Identity(), Identity(), hstack=False)) == \
        "CombineOperatorND(Identity,Identity, hstack=False)"
    X = [np.arange(6.0).reshape(2, 3), np.ones((2, 3))]
    for hstack, shape in ((True, (2, 6)), (False, (4, 3))):
        nd = CombineOperatorND(Identity(), Identity(), hstack)
        out = nd.compute(X, None)
        assert [o.shape for o in out] == [shape, shape] and np.array_equal(nd.extract(X[0]), out[0])
        assert sorted(nd.__dict__) == ["_hstack", "model1", "model2"]
    flat = CombineOperator(Identity(), Identity())
    stack = flat.compute(np.stack(X), None)          # an array [n][H][W] on the plain path (it has a .device too)
    assert len(stack) == 2 and np.array_equal(stack[1], np.ones((1, 12)))
    assert np.array_equal(flat.compute(X, None)[0], np.hstack((X[0].reshape(1, -1), X[0].reshape(1, -1))))
    assert flat.extract(X[1]).shape == (1, 12) and sorted(flat.__getstate__()) == ["model1", "model2"]
