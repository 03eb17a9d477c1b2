#!/usr/bin/env python3
"""Build gate (recnext_amd/csrc/Makefile): list every kernel of the given hipcc -S listings with its register and scratch figures and fail
when a kernel the DEFAULT dispatch reaches has a private segment (registers spilled to memory).  Default dispatch = the inference
instantiations for bf16 / float32 activations of the fused kernels (k_recconv_cpt without TRAIN, k_recconv_cpl14, k_recconv_cpl7b) and the
tiled step kernels (k_upadd_cpt, k_down5_cpt, k_down7m2_cpt), and every instantiation of the input adjoint (k_recconv_adj_cpl14,
k_recconv_adj_cpl7), and RecAttn2d's wide-head attention kernels (k_recattn_short_w, k_recattn_kv_w, k_recattn_out_w: every instantiation), and the
channel mixer's kernels (k_channel_mlp, k_channel_mlp_stream, k_channel_mlp_pair, k_channel_mlp_res128, k_channel_mlp_wide; the 320-channel stream kernel is reported only), and the
backward of the T / S / B grouped Downsample conv (k_ls_down_gx, k_ls_down_gw: every instantiation), and the training step's BatchNorm (rcx_bn.hip's k_bn_*: every instantiation) and its one-operator RepVGGDW (rcx_repdw.hip's k_rep_*: every instantiation) and depthwise ConvNorm (rcx_dwbn.hip's k_dwbn_*: every instantiation) and the channel mixers' BatchNorm with its GELU or residual epilogue (rcx_bnact.hip's k_bnact_*: every instantiation), and the classifier head (rcx_head.hip's k_head_*: every instantiation); the
training-forward and float16 instantiations and the other matrix-core attention kernels (rcx_qkcore's 32-wide and padded heads) are reported only.
usage: check_scratch.py file.s [file.s ...]"""
import re
import subprocess
import sys


def demangle(names):
    try:
        for tool in ("c++filt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"):
            try:
                out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
                return out.strip().split("\n")
            except FileNotFoundError:
                continue
    except Exception:
        pass
    sys.exit("check_scratch.py: no demangler (c++filt / llvm-cxxfilt): cannot tell the gated kernels apart")


bad = 0
rows = []
for path in sys.argv[1:]:
    cur = {}
    for line in open(path):
        m = re.match(r"\s+\.(name|private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\S+)", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if k == "name" and "name" in cur and "private_segment_fixed_size" in cur:
            rows.append((path, cur))
            cur = {}
        if k == "name" and re.match(r"^_Z", v) is None:
            continue                                       # argument names of the metadata, not the kernel symbol
        cur[k] = v
        if all(x in cur for x in ("name", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")):
            rows.append((path, cur))
            cur = {}
names = demangle([r[1]["name"] for r in rows])
for (path, r), name in zip(rows, names):
    priv = int(r["private_segment_fixed_size"])
    short = re.sub(r"^void rcx::", "", name)
    short = re.sub(r"\(.*$", "", short)
    fp16 = "_Float16" in short or "DF16_" in short
    # template arguments of k_recconv_cpt: <T, HALVES, MODE, PIXB, TIO, TRAIN, LV, STG>
    m = re.match(r"cpt::k_recconv_cpt<(\d+), (\d+), (\d+), (\d+), ([^,]+), (true|false), ", short)
    gated = False
    if m:
        gated = m.group(6) == "false" and not fp16
    elif re.match(r"(cpl14::k_recconv_cpl14|cpl14::k_recconv_cpl7b|cpl14::k_upadd_cpl14|cpl14::k_upadd_cpl7|cpl14::k_down5_cpl7|upcpt::k_upadd_cpt|upcpt::k_down5_cpt|upcpt::k_down7m2_cpt)<", short):
        gated = not fp16
    elif re.match(r"cpladj::k_recconv_adj_cpl(14|7)<", short):
        gated = True                                       # the input adjoint: every instantiation, float16 included, is default dispatch
    elif re.search(r"k_recattn_(short|kv|out)_w(<|I)", short):
        gated = True                                       # wide heads (36 .. 64 channels): every instantiation, float16 x included (mangled when undemangled)
    elif re.search(r"\dk_lt_(rep|kv|out|conv)I", r["name"]):
        gated = True                                       # the tiled T / S / B token half: every instantiation (by the mangled name: the
        m = re.search(r"k_lt_\w+<[^(]*>", name)                        # kernels of an anonymous namespace lose theirs to the cut above)
        short = short or (m.group(0) if m else name)
    elif re.search(r"\dk_ls_down_g[xw]I", r["name"]):
        gated = True                                       # the grouped Downsample conv's backward: every instantiation
        m = re.search(r"k_ls_down_g[xw]<[^(]*>", name)
        short = short or (m.group(0) if m else name)
    elif re.search(r"3rcx2bn\d+k_bn_", r["name"]):
        gated = True                                       # the training step's BatchNorm (rcx_bn.hip): every instantiation, by the mangled name (float16 stays mangled)
    elif re.search(r"3rcx5repdw\d+k_rep_", r["name"]):
        gated = True                                       # RepVGGDW of a training step (rcx_repdw.hip): every instantiation, by the mangled name
    elif re.search(r"3rcx4dwbn\d+k_dwbn_", r["name"]):
        gated = True                                       # a depthwise ConvNorm of a training step (rcx_dwbn.hip): every instantiation, by the mangled name
    elif re.search(r"3rcx5bnact\d+k_bnact_", r["name"]):
        gated = True                                       # the channel mixers' BatchNorm + GELU / + residual of a training step (rcx_bnact.hip): every instantiation
    elif re.search(r"3rcx4head\d+k_head_", r["name"]):
        gated = True                                       # the classifier head (rcx_head.hip): every instantiation, by the mangled name
    elif re.match(r"mlp::k_channel_mlp(_pair|_stream|_res128|_wide)?<", short):
        # the channel mixer: every instantiation but the 320-channel stream kernel (ZPF off), whose 15 spilled registers sit outside its hidden-tile loop
        gated = not (short.startswith("mlp::k_channel_mlp_stream<") and short.endswith(", false>"))
    flag = ""
    if priv:
        flag = "  <-- SCRATCH" + (" (gated)" if gated else " (reported only)")
        bad += 1 if gated else 0
    print(f"{priv:5d} B scratch  {r['vgpr_count']:>3} VGPRs  {r['vgpr_spill_count']:>3} VGPR / {r['sgpr_spill_count']:>3} SGPR spills  {short}{flag}")
print(f"kernels: {len(rows)}  gated kernels with scratch: {bad}")
sys.exit(1 if bad else 0)
