"""The compiled k_shade, read from the built kernels_render.o: what reaches the vector-memory path and what spills.

k_shade waits for its turn in the CU's vector-memory pipeline, and its LDS copies of the scene tables and of the sky's marginal cdf are
there to keep lookups out of it.  They do only when the compiler knows the address space: a generic pointer chosen at run time turns
every lookup into a FLAT access, which is issued to the vector-memory side as well.  So the address space is fixed per instantiation
(k_shade<COUNT, LOD, TABLES, SKY>), and this file checks that the compiler still does what the source asks for:
  * no instantiation holds a FLAT access: LDS copies are read with ds_read, tables in memory with global_load;
  * the product instantiation spills no more registers than the build with generic pointers did (10)."""
import collections
import os
import re
import subprocess

import pytest

from conftest import ROOT

OBJ = os.path.join(ROOT, "glaze_amd", "csrc", "build", "kernels_render.o")
LLVM = "/opt/rocm/lib/llvm/bin"
PRODUCT = "_ZN3glz7k_shadeILb0ELb0ELb1ELb1EEEvNS_10LaunchArgsE"     # no counters, no texture LOD, tables and sky in LDS: what bench.py's atrium runs

pytestmark = pytest.mark.skipif(not (os.path.exists(OBJ) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))),
                                reason="kernels_render.o is not built (an object file of the in-tree build) or llvm-objdump is missing")


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isa")
    with open(OBJ, "rb") as f:
        (tmp / "in.o").write_bytes(f.read())
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", "in.o"], cwd=tmp, stdout=subprocess.DEVNULL)
    elf = [p for p in os.listdir(tmp) if "gfx950" in p]
    assert len(elf) == 1, elf
    return str(tmp / elf[0])


@pytest.fixture(scope="module")
def shade_kernels(code_object):
    """{mangled name: Counter of mnemonics} of every k_shade instantiation"""
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", code_object], text=True)
    kernels, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = kernels.setdefault(m.group(1), collections.Counter()) if "k_shadeI" in m.group(1) else None
        elif cur is not None and line.strip():
            cur[line.split()[0]] += 1
    return kernels


def test_every_instantiation_is_there(shade_kernels):
    assert len(shade_kernels) == 16 and PRODUCT in shade_kernels, sorted(shade_kernels)


def test_no_flat_access_in_any_k_shade(shade_kernels):
    for name, ops in shade_kernels.items():
        flat = {k: v for k, v in ops.items() if k.startswith("flat_load") or k.startswith("flat_store")}
        assert not flat, "%s: %s" % (name, flat)


def test_tables_in_lds_are_read_from_lds(shade_kernels):
    # the material scalars, the light and the texture descriptors are 16-byte reads: in LDS they are ds_read_b128, in memory global_load_dwordx4
    for lod in "01":
        res, mem = (shade_kernels["_ZN3glz7k_shadeILb0ELb%sELb%sELb1EEEvNS_10LaunchArgsE" % (lod, t)] for t in "10")
        assert res["ds_read_b128"] > mem["ds_read_b128"] and res["global_load_dwordx4"] < mem["global_load_dwordx4"]


def test_product_kernel_spills_no_more_than_before(code_object):
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", code_object], text=True)
    spill, name = {}, None
    # the metadata lists a kernel's fields alphabetically: .name comes before .vgpr_spill_count
    for line in notes.split("\n"):
        m = re.match(r"\s*-?\s*\.name:\s*(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s*-?\s*\.vgpr_spill_count:\s*(\d+)", line)
        if m and name:
            spill[name] = int(m.group(1))
    assert spill[PRODUCT] <= 10, spill[PRODUCT]
