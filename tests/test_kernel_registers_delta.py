"""Register budget of the delta-scatter loop's kernels, by the rule of tests/test_kernel_registers.py (no GPU): the stencil
kernel on the plain plane, k_stencil_binned<HS, 3, 256>, stays at <= 80 scalar registers without a spill -- 8 waves per SIMD
beside the other contexts' kernels -- and so does the scatter kernel k_warp_scatter_delta."""
import os

import pytest

from test_kernel_registers import kernel_table


@pytest.fixture(scope="module")
def built():
    from better_flow_amd import accel
    assert os.path.exists(accel.LIB_PATH), "the library is not built: %s" % accel.LIB_PATH
    return kernel_table(accel.LIB_PATH)


@pytest.mark.parametrize("hs", range(5))
def test_stencil_plane_budget(built, hs):
    name = "bf::k_stencil_binned<%d,3,256>" % hs
    assert name in built, "%s is not in the library" % name
    r = built[name]
    print(name, r)
    assert r["sgpr_count"] <= 80
    assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0
    if hs == 1:   # the headline's: the dense-slab form's bars (test_stencil_dense_budget)
        assert r["vgpr_count"] <= 64
        assert r["private_segment_fixed_size"] <= 64
        assert r["group_segment_fixed_size"] <= 18720


@pytest.mark.parametrize("packed", ("true", "false"))
def test_scatter_delta_budget(built, packed):
    names = [k for k in built if k.startswith("bf::k_warp_scatter_delta<%s," % packed)]   # (<PACKED, events per thread>)
    assert len(names) == 1, names
    name = names[0]
    r = built[name]
    print(name, r)
    assert r["sgpr_count"] <= 80
    assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0
    assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0
