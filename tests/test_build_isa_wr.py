"""The register budget of conv_wh.h's 160-channel kernel (conv_wr_kernel), checked on the compiler's own output (no GPU),
the way test_build_isa.py checks the 80-channel kernel: 512-thread workgroups (two waves per SIMD: 256 registers per lane)
holding 160 row accumulators, the U ring, the A fragments and one set of products -- a spill would pass every parity test
and cost tens of percent.  The multiplying chunk loop must hold 4 frequencies x 10 column tiles x 4 terms = 160 MFMAs of
the binary16 shape in ONE basic block (the U refills and the row adds are pinned between them; a branch inside would break
that order), every one of the first two of a column tile starting from C = 0.
(The form that accumulates the rows inside the MFMAs -- 240 per chunk, the count this test was first written for -- was
built and measured: it is 1.15-1.27 x less accurate than the 80-channel kernel and fails test_gpu_fullrank's block gate;
profiles/NOTES_r30.md.)"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

TU_WR = """
#include "conv_wh.h"
namespace sinddm {
ConvProfiler& conv_profiler() { static ConvProfiler p; return p; }
int touch_wr(const ConvArgs& a, hipStream_t st) { return conv_wh_launch(a, st, 2); }
}
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_160_channel_kernel_fits_its_register_budget():
    from sinddm_amd import build
    tmp = tempfile.mkdtemp(prefix="wrisa")
    try:
        src = os.path.join(tmp, "t.hip")
        with open(src, "w") as f:
            f.write(TU_WR)
        flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared")]
        subprocess.check_call([HIPCC, *flags, "-I", os.path.join(ROOT, "include"), "-I", build.CSRC,
                               "--cuda-device-only", "-S", src, "-o", os.path.join(tmp, "t.s")],
                              stderr=subprocess.DEVNULL)
        s = open(os.path.join(tmp, "t.s")).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    meta = {}
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size: +\d+", s, re.S):
        name = re.search(r"\.name: +(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s: +(\d+)" % k, blk).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "max_flat_workgroup_size")}
    wr = [k for k in meta if "conv_wr_kernel" in k]
    assert len(wr) == 1, sorted(meta)
    m = meta[wr[0]]
    assert m["max_flat_workgroup_size"] == 512 and m["vgpr_count"] <= 256, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    body = s[s.index(wr[0] + ":"):]
    body = body[:body.index(".Lfunc_end")]
    lines = [l.strip() for l in body.split("\n") if l.strip() and not l.strip().startswith(";")]
    assert not [l for l in lines if l.startswith("scratch_")]
    assert not [l for l in lines if l.startswith("v_mfma") and "v_mfma_f32_16x16x32_f16" not in l]
    # basic blocks by label: the chunk loop of the multiplying instantiation holds all 160, nothing else holds any
    counts, cur = [], 0
    for l in lines:
        if re.match(r"^\.LBB\d+_\d+:", l):
            counts.append(cur)
            cur = 0
        elif l.startswith("v_mfma_f32_16x16x32_f16"):
            cur += 1
    counts.append(cur)
    assert [c for c in counts if c] == [160], [c for c in counts if c]
    # the products start from zero: half of the MFMAs take the inline constant as C
    assert sum(l.startswith("v_mfma") and l.endswith(", 0") for l in lines) == 80
    # the service instantiation: the same transform as the 80-channel kernel (two copies: first chunk and chunk loop)
    assert body.count("v_mov_b32_dpp") == 64 and body.count("v_fma_mixlo_f16") == 96 and body.count("v_fma_mixhi_f16") == 96
