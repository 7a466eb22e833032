"""What the compiler made of the cigar text kernels (csrc/npr_cigtext.hip), read from its assembly (no GPU needed: hipcc cross-compiles):
no private segment, no scratch traffic, every store to memory a vector store, and registers and LDS small enough that the wavefront slots
bound the occupancy (eight wavefronts per SIMD: 64 VGPRs; k_cigtext_write's tile buffer is its only LDS)."""
import re

import pytest

from test_isa_budget import _asm_of, _kernel_meta

# (the three passes of the offsets are the int64 instances of the shared scan, csrc/npr_scan.h, compiled in npr_scan.hip)
KERNELS = ["13k_cigtext_len", "16k_scan_tile_sumsIllEE", "12k_scan_groupIllEE", "12k_scan_tilesIllEE", "15k_cigtext_write"]


@pytest.fixture(scope="module")
def cigtext_asm(tmp_path_factory):
    return _asm_of(tmp_path_factory, "npr_cigtext.hip") + _asm_of(tmp_path_factory, "npr_scan.hip")


@pytest.mark.parametrize("name", KERNELS)
def test_cigar_text_kernels_keep_their_budget(cigtext_asm, name):
    vgpr, scratch, lds = _kernel_meta(cigtext_asm, name)
    assert vgpr <= 64, (name, vgpr)
    assert scratch == 0, (name, scratch)
    assert lds <= (2820 if name.endswith("write") else 64), (name, lds)
    m = re.search(r"\n(_ZN\S*%s\S*):.*?s_endpgm" % re.escape(name), cigtext_asm, re.S)
    assert m, name
    instrs = [ln.split()[0] for ln in m.group(0).split("\n") if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
    assert len(instrs) > 20, name
    assert not [i for i in instrs if i.startswith("scratch_")], name
    # every write to memory goes through the vector unit: no scalar-unit instruction that stores, adds to memory or writes its cache back
    assert not [i for i in instrs if re.match(r"s_\w*(store|atomic|dcache)", i)], name
    assert not [i for i in instrs if "atomic" in i], name


def test_text_leaves_as_whole_dwords(cigtext_asm):
    m = re.search(r"\n(_ZN\S*15k_cigtext_write\S*):.*?s_endpgm", cigtext_asm, re.S)
    body = m.group(0)
    assert "global_store_dword " in body and "global_store_byte" in body and "ds_write_b8" in body
