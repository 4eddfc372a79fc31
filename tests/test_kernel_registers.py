"""Register budget of the two loop kernels, read from the gfx950 code objects of the library the tests load (no GPU).

A CU admits floor(800 / (ceil(sgpr / 16) * 16 + 16)) waves per SIMD, at most 8: 8 waves up to 80 scalar registers, 7 up to
96, 6 up to 112.  The scatter kernel (K1, k_bin_warp_scatter_lean<W, 512, U, 0>) and the stencil kernel (K3,
k_stencil_binned<1, 0, 256>) of the co-scheduled dense loop are held to <= 80 WITHOUT spills; every other instantiation of
k_bin_warp_scatter / k_bin_warp_scatter_lean / k_stencil_binned / k_stencil_binned_full is held to "no worse than the parent
commit" in the five numbers recorded in tests/kernel_registers_parent.txt.

The numbers are the `.sgpr_count`, `.sgpr_spill_count`, `.vgpr_count`, `.vgpr_spill_count`, `.private_segment_fixed_size` and
`.group_segment_fixed_size` entries of the code objects' metadata note (llvm-readelf --notes).  No instruction is looked at.

`python tests/test_kernel_registers.py <library>` prints the table in the format of kernel_registers_parent.txt.
"""
import os
import re
import subprocess
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PARENT_TABLE = os.path.join(HERE, "kernel_registers_parent.txt")
FIELDS = ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")
FAMILIES = ("bf::k_bin_warp_scatter<", "bf::k_bin_warp_scatter_lean<", "bf::k_stencil_binned<", "bf::k_stencil_binned_full<")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _rocm_tool(name):
    roots = [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    for r in roots:
        if not r:
            continue
        for sub in ("llvm/bin", "lib/llvm/bin", "bin"):
            p = os.path.join(r, sub, name)
            if os.path.exists(p):
                return p
    raise AssertionError("%s not found under the ROCm tree" % name)


def _code_objects(lib):
    """The gfx950 code objects of every offload bundle in the library's fat binary (one bundle per source file)."""
    data = open(lib, "rb").read()
    out = []
    for m in re.finditer(re.escape(BUNDLE_MAGIC), data):
        base = m.start()
        pos = base + len(BUNDLE_MAGIC)
        n = int.from_bytes(data[pos:pos + 8], "little")
        pos += 8
        for _ in range(n):
            off, size, tlen = (int.from_bytes(data[pos + 8 * i:pos + 8 * i + 8], "little") for i in range(3))
            triple = data[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if "gfx950" in triple and size:
                out.append(data[base + off:base + off + size])
    return out


def kernel_table(lib):
    """{demangled kernel name: {field: value}} for every kernel of the library."""
    readelf = _rocm_tool("llvm-readelf")
    objs = _code_objects(lib)
    assert objs, "no gfx950 code object in %s" % lib
    table = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, blob in enumerate(objs):
            path = os.path.join(tmp, "co%d.elf" % i)
            with open(path, "wb") as f:
                f.write(blob)
            notes = subprocess.run([readelf, "--notes", path], check=True, capture_output=True, text=True).stdout
            # one "- .agpr_count: ..." block per kernel inside amdhsa.kernels; keys of a block are in alphabetical order
            for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
                name = re.search(r"\n\s+\.name:\s+(\S+)", block)
                if not name:
                    continue
                rec = {}
                for fld in FIELDS:
                    v = re.search(r"\n\s+\.%s:\s+(\d+)" % fld, block)
                    rec[fld] = int(v.group(1)) if v else 0   # (the spill counts are omitted when zero)
                table[name.group(1)] = rec
    out = {}
    for n, rec in table.items():
        # _ZN2bf<len>k_nameI(Lb1E|Li512E)...EEv...: the kernel's name and its template arguments (bool / int literals only)
        m = re.match(r"_ZN2bf\d+(k_[a-z_0-9]+?)I((?:L[bi]\d+E)+)E", n)
        if m:
            args = [("true" if v == "1" else "false") if t == "b" else v for t, v in re.findall(r"L([bi])(\d+)E", m.group(2))]
            out["bf::%s<%s>" % (m.group(1), ",".join(args))] = rec
        else:
            out[n] = rec
    return out


def loop_kernels(lib):
    return {k: v for k, v in kernel_table(lib).items() if k.startswith(FAMILIES)}


def format_table(tab):
    lines = ["# kernel " + " ".join(FIELDS)]
    for k in sorted(tab):
        lines.append(k + " " + " ".join(str(tab[k][f]) for f in FIELDS))
    return "\n".join(lines) + "\n"


def read_parent():
    tab = {}
    for line in open(PARENT_TABLE):
        if line.startswith("#") or not line.strip():
            continue
        w = line.split()
        tab[w[0]] = dict(zip(FIELDS, (int(x) for x in w[1:])))
    return tab


@pytest.fixture(scope="module")
def built():
    from better_flow_amd import accel
    assert os.path.exists(accel.LIB_PATH), "the library is not built: %s" % accel.LIB_PATH
    return loop_kernels(accel.LIB_PATH)


K1_VGPR_MAX = {(True, 12): 76, (True, 10): 68, (True, 8): 60, (False, 12): 72, (False, 10): 64, (False, 8): 56}


@pytest.mark.parametrize("warp,per_thread", sorted(K1_VGPR_MAX))
def test_scatter_lean_dense_budget(built, warp, per_thread):
    name = "bf::k_bin_warp_scatter_lean<%s,512,%d,0>" % ("true" if warp else "false", per_thread)
    assert name in built, "%s is not in the library" % name
    r = built[name]
    print(name, r)
    assert r["sgpr_count"] <= 80
    assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0
    assert r["private_segment_fixed_size"] == 0
    assert r["vgpr_count"] <= K1_VGPR_MAX[(warp, per_thread)]


def test_stencil_dense_budget(built):
    name = "bf::k_stencil_binned<1,0,256>"
    assert name in built, "%s is not in the library" % name
    r = built[name]
    print(name, r)
    assert r["sgpr_count"] <= 80
    assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0
    assert r["vgpr_count"] <= 64
    assert r["private_segment_fixed_size"] <= 64
    assert r["group_segment_fixed_size"] <= 18720


def test_no_instantiation_worse_than_parent(built):
    parent = read_parent()
    assert len(parent) >= 100, "the parent table is incomplete"
    missing = sorted(set(parent) - set(built))
    assert not missing, "kernels of the parent commit that the library lacks: %s" % missing[:5]
    worse = []
    for k in sorted(parent):
        for f in FIELDS:
            if built[k][f] > parent[k][f]:
                worse.append("%s %s %d > %d" % (k, f, built[k][f], parent[k][f]))
    assert not worse, "\n".join(worse)


if __name__ == "__main__":
    sys.stdout.write(format_table(loop_kernels(sys.argv[1])))
