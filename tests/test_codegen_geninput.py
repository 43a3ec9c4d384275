"""Both instantiations of generator_input_kernel (csrc/geninput/generator_input.hip: the straight copy, the tile through LDS) in the built
library's gfx950 code object: present, no scratch, no spills, few registers, and exactly the LDS of one 64 x 65 float tile in the
transposing form and none in the other (no GPU; the code-object reader of tests/test_codegen_invariants.py).  Registers, scratch and
LDS bytes only."""
import re
import subprocess

from test_codegen_invariants import LLVM, code_objects  # noqa: F401  (the module-scoped fixture)

TILE = 64


def _kernel_notes(code_objects, sym):  # noqa: F811
    notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", code_objects["meta"][sym]["file"]], check=True, capture_output=True, text=True).stdout
    blk = next(b for b in re.split(r"\n\s+- \.agpr_count:|\n\s+- \.args:", notes) if re.search(r"\.name:\s+" + re.escape(sym) + r"\s", b))
    return {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
            for k in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count")}


def test_generator_input_kernels_registers_scratch_and_lds(code_objects):  # noqa: F811
    meta = code_objects["meta"]
    syms = sorted(k for k in meta if "generator_input_kernel" in k)
    assert len(syms) == 2 and "ILb0E" in syms[0] and "ILb1E" in syms[1], syms
    for sym, lds in zip(syms, (0, TILE * (TILE + 1) * 4)):
        n = _kernel_notes(code_objects, sym)
        assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0 and n["sgpr_spill_count"] == 0, (sym, n)
        assert n["group_segment_fixed_size"] == lds, (sym, n)          # 16 640 bytes: nine blocks of 256 threads fit a CU's 160 KiB
        assert n["vgpr_count"] <= 32 and n["sgpr_count"] <= 96, (sym, n)   # a copy kernel: nothing here may cost occupancy
