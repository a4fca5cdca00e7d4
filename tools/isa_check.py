"""ISA invariants of the persistent ping-pong kernels, checked on the compiler's output (no GPU needed):

  1. no `s_waitcnt vmcnt(0)` directly in front of the hand-written fragment reads (ds_read_b128 asm blocks) of a K loop.  hipcc's wait-count
     pass puts one there when it believes a compiler-visible VMEM operation may still be pending at the loop header (an epilogue load whose
     result is only read inside a conditional region, a visible store, ...); it drains the LDS-DMA prefetch ring in front of EVERY K-tile.
     Round 4 found it in the EPI_F32X kernels (present since round 3) and in a rewritten EPI_RESID epilogue (-3 % on fc2 / out-proj).
  2. no scratch memory beyond a few spilled registers (an accumulator array that a non-inlined lambda takes by reference lives in scratch).
  3. the attention kernels (attn_fwd*, attention.hip) use no scratch at all: their Q fragments and O accumulators are sized to the register
     file (attn_fwd96: 136 VGPRs, no AGPRs), and one spilled accumulator costs a scratch round trip per key tile.

  4. the gated (SwiGLU, EPI_GATED = 7) instantiations of both persistent GEMMs exist and obey 1 and 2 with NO scratch at all: their epilogue adds
     no row loads, so a spill there would be a regression of the epilogue itself.

  5. the RMSNorm / QK-norm kernels of the InternViT towers (rowops.hip: rms_rows, rms_stats_rows, rms_stats_finalize_rows, qk_rmsnorm_rows,
     rms_f32_rows; gemm_bf16.hip: splitk_reduce_rms) exist and use no scratch: a row of up to 4096 columns lives in 64 registers per lane.

  6. the ConvNeXt kernels (dwconv.hip: both dwconv7x7_stats_tile shapes, ln_stats_finalize_rows_odd, ln_space_to_depth2_rows) exist and use no
     scratch: 64 accumulators + 56 weights per lane (dwconv), a row of up to 4096 columns in 64 registers (space-to-depth).

  7. the SAM kernels (attention_relpos.hip: attn_fwd_relpos, relpos_tables_rows, the two sam_window_partition kernels and
     sam_window_unpartition_rows) exist and use no scratch: the position tables live in LDS, never in an indexed register array.

usage: python tools/isa_check.py [--sizes] [file.hip ...]      (default: the product library's persistent kernels)
--sizes also prints every kernel's code length (to compare the existing instantiations with a parent build)."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "law_of_vision_representation_in_mllms_amd", "csrc")
SIZES = "--sizes" in sys.argv[1:]
FILES = [a for a in sys.argv[1:] if a != "--sizes"] or ["gemm_bf16_v5.hip", "gemm_bf16_v2.hip", "ascore.hip", "attention.hip", "rowops.hip", "gemm_bf16.hip", "dwconv.hip", "attention_relpos.hip"]
# kernels (by name fragment) that must not touch scratch; Li7E = template argument EPI_GATED of gemm_bf16_256q / gemm_bf16_256
RMS_KERNELS = ("8rms_rows", "14rms_stats_rows", "23rms_stats_finalize_rows", "15qk_rmsnorm_rows", "12rms_f32_rows")
CONVNEXT_KERNELS = ("20dwconv7x7_stats_tileILi8ELi8EE", "20dwconv7x7_stats_tileILi16ELi16EE", "26ln_stats_finalize_rows_odd", "23ln_space_to_depth2_rows")
SAM_KERNELS = ("15attn_fwd_relpos", "18relpos_tables_rows", "23sam_window_partition_qk", "23sam_window_partition_vt", "27sam_window_unpartition_rows")
NO_SCRATCH = ("attn_fwd", "gemm_bf16_256qILi7E", "gemm_bf16_256ILi7E", "17splitk_reduce_rms") + RMS_KERNELS + CONVNEXT_KERNELS + SAM_KERNELS
REQUIRED = {"gemm_bf16_v5.hip": ("gemm_bf16_256qILi7ELb1E", "gemm_bf16_256qILi7ELb0E"), "gemm_bf16_v2.hip": ("gemm_bf16_256ILi7E",),
            "rowops.hip": RMS_KERNELS, "gemm_bf16.hip": ("17splitk_reduce_rms",), "dwconv.hip": CONVNEXT_KERNELS, "attention_relpos.hip": SAM_KERNELS}
bad = 0
for f in FILES:
    with tempfile.NamedTemporaryFile(suffix=".s") as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "--cuda-device-only", "-S",
               os.path.join(CSRC, f), "-o", tmp.name]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr[-2000:])
        lines = open(tmp.name).read().splitlines()
    kernel, wait_at = None, None
    hits, scratch, size = {}, {}, {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            kernel = m.group(1)
        t = ln.strip()
        if t.startswith("s_waitcnt vmcnt(0)"):
            wait_at = i
        elif t.startswith("ds_read_b128"):
            if wait_at is not None and i - wait_at <= 2 and "ASMSTART" in lines[i - 1]:
                hits[kernel] = hits.get(kernel, 0) + 1
            wait_at = None
        m = re.search(r"\.private_segment_fixed_size:\s*(\d+)", ln) or re.search(r"; ScratchSize: (\d+)", ln)
        if m and kernel:
            scratch[kernel] = max(scratch.get(kernel, 0), int(m.group(1)))
        m = re.search(r"; codeLenInByte = (\d+)", ln)
        if m and kernel:
            size[kernel] = int(m.group(1))
    for frag in REQUIRED.get(os.path.basename(f), ()):
        if not any(frag in k for k in scratch):
            print(f"{f}: no kernel matching {frag} (a required instantiation is missing)")
            bad += 1
    if SIZES:
        for k in sorted(size):
            print(f"{f}: {k}: {size[k]} bytes of code, {scratch.get(k, 0)} bytes of scratch")
    for k, n in hits.items():
        print(f"{f}: {k}: {n} K-loop header(s) behind s_waitcnt vmcnt(0)")
        bad += 1
    for k, n in scratch.items():
        if n > (0 if any(t in k for t in NO_SCRATCH) else 128):
            print(f"{f}: {k}: {n} bytes of scratch per lane")
            bad += 1
    print(f"{f}: {len(scratch)} kernels checked")
sys.exit(1 if bad else 0)
