"""The compiled k_trace, read from the built kernels_render.o: the machine-code budgets of the instantiation bench.py's atrium runs.

k_trace<false, kAlphaNone> is bound by VALU issue and is compiled for six waves per SIMD (GLZ_TRACE_WAVES), which leaves a lane 80
registers; a register spilt inside the traversal loops costs scratch traffic on every node visit, and six blocks fit a CU only while a
block's LDS (17 stack levels, the link and work-sharing scratch, the staged tree top) stays at 25 920 bytes.  Only the code object's
metadata (llvm-readelf --notes) is read here, no instruction."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

OBJ = os.path.join(ROOT, "glaze_amd", "csrc", "build", "kernels_render.o")
LLVM = "/opt/rocm/lib/llvm/bin"
PRODUCT = "_ZN3glz7k_traceILb0ELi0EEEvNS_10LaunchArgsE"     # no counters, no alpha code: a scene without opacity maps

pytestmark = pytest.mark.skipif(not (os.path.exists(OBJ) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))),
                                reason="kernels_render.o is not built (an object file of the in-tree build) or llvm-objdump is missing")


@pytest.fixture(scope="module")
def kernel_metadata(tmp_path_factory):
    """{mangled kernel name: {metadata field: int}} of the gfx950 code object inside kernels_render.o"""
    tmp = tmp_path_factory.mktemp("isa")
    with open(OBJ, "rb") as f:
        (tmp / "in.o").write_bytes(f.read())
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", "in.o"], cwd=tmp, stdout=subprocess.DEVNULL)
    elf = [p for p in os.listdir(tmp) if "gfx950" in p]
    assert len(elf) == 1, elf
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp / elf[0])], text=True)
    # amdhsa.kernels is a list with one item per kernel: a dash at the list's own indentation opens an item, and its fields sit two
    # columns further in (the items of a kernel's .args list are indented deeper and are skipped)
    kernels, cur, dash = {}, None, None
    for line in notes.split("\n"):
        if line.strip() == "amdhsa.kernels:":
            dash = -1
            continue
        if dash is None:
            continue
        m = re.match(r"(\s*)(- |  )\.(\w+):\s*(\S*)", line)
        if not m:
            if line.strip() and not line.startswith(" "):
                dash = None     # the next top-level key: the list has ended
            continue
        col = len(m.group(1))
        if dash == -1 and m.group(2) == "- ":
            dash = col
        if col != dash:
            continue
        if m.group(2) == "- ":
            cur = {}
        if m.group(3) == "name":
            kernels[m.group(4)] = cur
        elif re.fullmatch(r"\d+", m.group(4)):
            cur[m.group(3)] = int(m.group(4))
    return kernels


def test_every_k_trace_instantiation_is_there(kernel_metadata):
    names = sorted(k for k in kernel_metadata if "k_traceI" in k)
    assert len(names) == 3 and PRODUCT in names, names


def test_product_k_trace_keeps_its_budgets(kernel_metadata):
    k = kernel_metadata[PRODUCT]
    print("k_trace<false, kAlphaNone>:", k)
    assert k["vgpr_count"] <= 80, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] <= 25920, k
