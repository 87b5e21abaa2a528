"""CPU side of tests/test_hip_consumers.py (tests/_consumers.py): the references are what they claim to be.

1. The oracle itself satisfies the centroid identity on every case the GPU file pools side tensors on: in weighted mode its pooled row
   is the float64 mean of the side tensor over the tokens that ref_token_maps assigns to that output row, within what its own
   arithmetic can lose (rounding_bound: from the number formats and the chain lengths alone).  So the identity is the reference's
   definition (quadtree_builder.py:75-81, quadtree_temporal_merger.py:153-169), not this project's.
2. The oracle's largest deviation from the float64 centroid per side dtype is printed (pytest -s): twice that figure is the bar of the
   device's rows (profiles/consumers_on_every_path.md records it).
3. Every case is decisive: no spatial or temporal similarity lies within the band of tests/_offdist.py around its threshold.
"""
import pytest
import torch

from tests import _consumers as C


@pytest.mark.parametrize("name", C.case_names(pos_only=True))
def test_oracle_satisfies_the_centroid_identity(name):
    c = C.cases()[name]
    ref = C.reference(name)
    maps = ref["maps"]
    assert int(maps["cover"].min()) == 1 and int(maps["cover"].max()) == 1, "every token belongs to exactly one node"
    assert torch.equal(torch.bincount(maps["token_to_out"].flatten().long()), maps["npatch"].long())
    bound = C.rounding_bound(c)
    for which, rows, c64 in zip(("coord", "rnd"), ref["pos_w"], ref["centroid"]):
        assert rows.dtype == c.side_dtype and rows.shape == c64.shape
        assert bool(torch.isfinite(rows).all()), f"{name}: the side tensor is finite, so are its pooled rows"
        if which == "coord":
            dev = C.deviation(rows, c64)
            print(f"{name} [{c.side_dtype}]: oracle vs float64 centroid {dev:.3e} (bound {bound:.3e})")
            assert dev <= bound, f"{name}: the oracle's weighted rows are not the centroid: {dev:.3e} > {bound:.3e}"
            assert torch.equal(rows[:, C.ONES].double(), torch.ones(rows.shape[0], dtype=torch.float64)), \
                f"{name}: sum of ones / num_patches must be exactly 1"
        else:
            # signed terms: the bound holds relative to the mean of |terms| <= 1, i.e. absolutely
            err = float((rows.double() - c64).abs().max())
            assert err <= bound, f"{name}: rnd rows {err:.3e} > {bound:.3e}"


def test_oracle_deviation_per_side_dtype():
    """The figure behind the device's bar: non-zero (a bar of zero would demand the oracle's summation order); its upper bound is
    the per-case assertion above."""
    for dtype in (torch.float32, torch.bfloat16):
        dev = C.oracle_deviation(dtype)
        n = sum(1 for k in C.case_names(pos_only=True) if C.cases()[k].side_dtype == dtype)
        print(f"oracle's largest deviation from the float64 centroid, {dtype} side tensors ({n} cases): {dev:.3e}")
        assert dev > 0.0


@pytest.mark.parametrize("name", C.case_names())
def test_every_case_is_decisive(name):
    b = C.band(C.cases()[name])
    print(f"{name}: {b.n_decisions} decisions, eps spatial {b.eps_sp:.2e} temporal {b.eps_tp:.2e}, in band {b.in_band}")
    assert b.n_decisions > 0
    assert b.nan_mismatch == 0, f"{name}: a similarity is NaN in one arithmetic only"
    assert b.decisive, f"{name}: {b.in_band} decisions inside the band -- pick another seed"


def test_side_tensor_channels():
    coord, rnd = C.side_tensors(3, 5, 7, 6, torch.float32)
    assert coord.shape == (3, 6, 5, 7) and coord.permute(0, 2, 3, 1).is_contiguous()
    assert coord[2, :, 4, 6].tolist() == [2.0, 4.0, 6.0, 1.0, 2 * 35 + 4 * 7 + 6, 0.0]
    assert float(rnd.min()) >= -1.0 and float(rnd.max()) < 1.0
    t2o = torch.tensor([[[0, 0], [1, 1]]], dtype=torch.int32)
    side = C.side_tensors(1, 2, 2, 5, torch.float32)[0]
    assert C.centroid64(side, t2o, 2).tolist() == [[0.0, 0.0, 0.5, 1.0, 0.5], [0.0, 1.0, 0.5, 1.0, 2.5]]
