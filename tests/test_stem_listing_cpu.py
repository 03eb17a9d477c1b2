"""What the compiler made of the one-launch stem at RecNeXt-M3's shape, read from this project's own gfx950 listing of rcx_stem.hip (no GPU needed):
k_stem<32, 32, 2, true, false> keeps no private segment, fits two waves per SIMD (at most 256 registers) and reads no bias from LDS between the tile loop's barriers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recnext_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNEL = "_ZN3rcx4stem6k_stemILi32ELi32ELi2ELb1ELb0EEEv"          # rcx::stem::k_stem<32, 32, 2, true, false>

# LDS instructions between barrier 1 and barrier 2 of the tile loop (phase A), as the source implies for M1 = 1, KC = 32:
#   2   ds_read_b128: the two W1 fragments (k-steps 0 and 1), once per tile, held in registers for the wave's three pixel tiles
#  48   ds_read_u16:  3 pixel tiles a wave (rounds 0 and 1 and the shared last round) x 2 k-steps x 8 im2col inputs
#   8   ds_write_b64: rounds 0 and 1, all four channel groups g (8 channels x bf16 = 16 bytes a pixel = 8 bytes a lane half h)
#   4   ds_write_b64: the shared last round, two channel groups a wave, once in the branch of each wave of a pair (even g | odd g)
# = 62, and none of them a bias read: the b1 quads are in registers from the prologue on (the parent had 12 ds_read_b128 of b1 here: 3 pixel tiles x 4 groups).
PHASE_A_LDS = {"ds_read_b128": 2, "ds_read_u16": 48, "ds_write_b64": 12}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("stem") / "rcx_stem.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Xclang", "-target-feature", "-Xclang", "-load-store-opt", "-I", CSRC,
           "--cuda-device-only", "-S", os.path.join(CSRC, "rcx_stem.hip"), "-o", str(out)]                   # the Makefile's CXXFLAGS, device side only
    subprocess.check_call(cmd)
    return out.read_text()


def _kernel_text(listing):
    # the label, the code up to s_endpgm, then the kernel descriptor and the compiler's "; Kernel info:" comments up to the next function's section
    m = re.search(r"^" + KERNEL + r"\w*:[^\n]*\n(.*?)^\s*s_endpgm\b(.*?; Occupancy:[^\n]*\n)", listing, re.S | re.M)
    assert m, "k_stem<32, 32, 2, true, false> is not in the listing"
    return m.group(1), m.group(2)


def test_m3_stem_kernel_has_no_scratch_and_two_waves_per_simd(listing):
    _, tail = _kernel_text(listing)
    scratch = int(re.search(r";\s*ScratchSize:\s*(\d+)", tail).group(1))
    total = int(re.search(r";\s*TotalNumVgprs:\s*(\d+)", tail).group(1))
    print(f"\nk_stem<32,32,2,true,false>: {total} registers, scratch {scratch}")
    assert scratch == 0 and re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", tail)
    assert total <= 256


def test_m3_stem_phase_a_reads_no_bias_from_lds(listing):
    body, _ = _kernel_text(listing)
    lines = [ln.split(";")[0].split() for ln in body.splitlines()]
    ops = [ln[0] for ln in lines if ln and not ln[0].endswith(":") and not ln[0].startswith(".")]
    bars = [i for i, op in enumerate(ops) if op == "s_barrier"]
    assert len(bars) == 2, bars                                      # the tile loop's two barriers; the prologue has none
    counts = {}
    for op in ops[bars[0]:bars[1]]:
        if op.startswith("ds_"):
            key = "ds_read_u16" if op.startswith("ds_read_u16") else op          # (the _d16 / _d16_hi forms write a register half: the same request)
            counts[key] = counts.get(key, 0) + 1
    print(f"\nphase A LDS instructions: {counts}")
    assert counts == PHASE_A_LDS
