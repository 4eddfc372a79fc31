"""The structs and the entry point of the coarse-to-fine per-cell search (include/bf_accel.h): ctypes mirrors against
sizeof() as compiled into the release library, and the exported symbol.  No compute calls."""
import ctypes


def test_pyramid_structs_match_header_sizes():
    from better_flow_amd import accel
    lib = ctypes.CDLL(accel.LIB_PATH)
    assert lib.bf_abi_struct_sizes(None, 0) == 10
    out = (ctypes.c_int32 * 12)(*([-1] * 12))
    assert lib.bf_abi_struct_sizes(out, 12) == 10 and list(out)[10:] == [-1, -1]
    assert list(out)[8:10] == [ctypes.sizeof(accel.GlobalPyramidOpts), ctypes.sizeof(accel.GlobalPyramidInfo)] == [12, 96]
    assert accel.GlobalPyramidInfo.level_count.offset == 24 and accel.GlobalPyramidInfo.levels_run.offset == 88
    first = (ctypes.c_int32 * 8)()
    assert lib.bf_abi_struct_sizes(first, 8) == 8 and list(first) == list(out)[:8]      # the list only grows at its end


def test_pyramid_symbol_is_exported():
    from better_flow_amd import accel
    lib = ctypes.CDLL(accel.LIB_PATH)
    assert hasattr(lib, "bf_global_search_cells_pyramid")
    assert "bf_global_search_cells_pyramid" in accel.EXPORTS
