"""tests/guard.py proved on CPU tensors: five planted faults, written as fake "ops" in Python, are each caught by the matching check and a correct op
passes; the proxy hands out exactly the shape, dtype, strides and alignment the real torch.empty / torch.empty_like would; and the case table of
tests/test_guard_bands_gpu.py names every launching entry of recnext_amd.ops and every schedule family the plan functions can return."""
import inspect
import os
import re
import sys

import pytest
import torch

from tests import guard

ME = sys.modules[__name__]          # guarded_library(modules=[ME]) replaces this module's own `torch`: the fake ops below allocate through it


# ---- the fake ops: y = 2 x on an (R, C) tensor ------------------------------------------------------------------------------------------------------------

def op_ok(x):
    y = torch.empty_like(x)
    y.copy_(x * 2)
    return y


def op_store_past_the_end(x):
    y = op_ok(x)
    y.as_strided((1,), (1,), y.storage_offset() + y.numel()).fill_(1.0)
    return y


def op_store_in_front(x):
    y = op_ok(x)
    y.as_strided((1,), (1,), y.storage_offset() - 1).fill_(1.0)
    return y


def op_last_row_unwritten(x):
    y = torch.empty_like(x)
    y[:-1].copy_(x[:-1] * 2)
    return y


def op_reads_past_its_input(x):
    y = op_ok(x)
    y[-1, -1] += x.as_strided((1,), (1,), x.storage_offset() + x.numel())[0] * 0.0       # "masked afterwards": 0 * garbage
    return y


def op_modifies_its_input(x):
    y = op_ok(x)
    x[0, 0] = 0.0
    return y


def _x(dtype=torch.float32):
    return (torch.arange(12, dtype=torch.float32).reshape(3, 4) + 1).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_a_correct_op_passes_all_checks(dtype):
    x = _x(dtype)
    y = guard.run_properties(op_ok, (x,), modules=[ME])
    assert torch.equal(y, x * 2)
    assert ME.torch is torch, "the module's own torch name is restored"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_a_store_one_element_past_the_output_is_caught(dtype):
    with guard.guarded_library([ME]) as rec:
        op_store_past_the_end(_x(dtype))
    n = 12 * _x(dtype).element_size()
    with pytest.raises(AssertionError, match=rf"empty_like #0 \(op_ok.*shape \(3, 4\) {re.escape(str(dtype))}.*offset {n} relative to the payload"):
        guard.check_guards(rec.arenas)


def test_a_store_one_element_in_front_of_the_output_is_caught():
    with guard.guarded_library([ME]) as rec:
        op_store_in_front(_x())
    with pytest.raises(AssertionError, match=r"offset -4 relative to the payload \(4 bytes changed in front"):
        guard.check_guards(rec.arenas)


def test_an_unwritten_last_row_is_caught():
    x = _x()
    with guard.guarded_library([ME]) as rec:
        y = op_last_row_unwritten(x)
    guard.check_guards(rec.arenas)                                   # nothing written outside: A holds, B does not
    with pytest.raises(AssertionError, match=r"4 NaN elements, the first at \(2, 0\)"):
        guard.check_written(y)
    with pytest.raises(AssertionError, match="differs in 4 elements"):
        guard.check_same(y, op_ok(x), "poisoned against plain")


def test_a_read_past_the_input_is_caught():
    x = _x()
    results = []
    for fill in (0x00, 0xFF):
        inputs = []
        gx = guard.guarded_copy(x, fill, inputs)
        with guard.guarded_library([ME]) as rec:
            results.append(op_reads_past_its_input(gx))
        guard.check_guards(rec.arenas + inputs)
        guard.check_inputs_unchanged(inputs)
    assert torch.equal(results[0], op_ok(x))                        # 0 * 0.0: the masked read is invisible with zeros behind the input ...
    with pytest.raises(AssertionError, match="NaN"):                # ... and a NaN with 0xFF behind it
        guard.check_written(results[1])
    with pytest.raises(AssertionError, match="differs in 1 elements"):
        guard.check_same(results[0], results[1], "0x00 against 0xFF")


def test_a_modified_input_is_caught():
    inputs = []
    gx = guard.guarded_copy(_x(), 0x00, inputs)
    op_modifies_its_input(gx)
    guard.check_guards(inputs)
    with pytest.raises(AssertionError, match=r"input modified: input #0 .*shape \(3, 4\) torch.float32.*offset 2 relative to the payload \(2 bytes changed"):    # 1.0f = 00 00 80 3f
        guard.check_inputs_unchanged(inputs)


@pytest.mark.parametrize("op", [op_last_row_unwritten, op_modifies_its_input])
def test_run_properties_fails_for_a_planted_fault(op):
    with pytest.raises(AssertionError):
        guard.run_properties(op, (_x(),), modules=[ME], repeat=False)
    assert ME.torch is torch


def test_an_aliased_argument_stays_one_tensor():
    x = _x()
    seen = []
    guard.map_tensors((x, [x, None, 3], x.clone()), lambda t: seen.append(t) or t)
    assert len(seen) == 2


# ---- the proxy hands out what the real call would ----------------------------------------------------------------------------------------------------------

def _same_layout(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.stride() == b.stride() and a.device == b.device


def test_proxy_preserves_strides_dtypes_and_alignment():
    from recnext_amd import ops
    x = torch.randn(2, 6, 5, 3).contiguous(memory_format=torch.channels_last)
    sliced = torch.randn(4, 6, 5, 3).contiguous(memory_format=torch.channels_last)[1:3]
    with guard.guarded_library() as rec:
        assert ops.torch is rec.proxy and ops.torch.float32 is torch.float32 and ops.torch.nn is torch.nn
        y = ops._empty_nhwc(2, 6, 5, 3, torch.bfloat16, "cpu")
        z = ops.torch.empty_like(x, memory_format=torch.channels_last)
        z2 = ops.torch.empty_like(sliced.bfloat16(), memory_format=torch.channels_last)
        q = ops.torch.empty_like(torch.randn(2, 15, 6))
        ws = ops.torch.empty(1001, dtype=torch.uint8, device="cpu")
        w2 = ops.torch.empty((3, 25 * 6), dtype=torch.float32, device="cpu")
        nothing = ops.torch.empty(0, dtype=torch.uint8, device="cpu")
        none_f32 = ops.torch.empty((0, 6), dtype=torch.float32, device="cpu")
    assert ops.torch is torch
    assert _same_layout(y, ops._empty_nhwc(2, 6, 5, 3, torch.bfloat16, "cpu")) and y.is_contiguous(memory_format=torch.channels_last)
    assert _same_layout(z, torch.empty_like(x, memory_format=torch.channels_last)) and z.stride() == (90, 1, 18, 6)
    assert _same_layout(z2, torch.empty_like(sliced.bfloat16(), memory_format=torch.channels_last))
    assert _same_layout(q, torch.empty(2, 15, 6)) and _same_layout(ws, torch.empty(1001, dtype=torch.uint8)) and _same_layout(w2, torch.empty(3, 150))
    assert nothing.numel() == 0 and none_f32.shape == (0, 6)
    assert [a.nbytes for a in rec.arenas] == [360, 720, 360, 720, 1001, 1800, 0, 0]
    for a in rec.arenas:
        assert a.buf.numel() == a.nbytes + 2 * guard.GUARD                                       # the tail guard starts at the payload's last byte
        if a.nbytes:                                                                             # (an empty tensor reports no address)
            assert a.tensor.data_ptr() == a.buf.data_ptr() + guard.GUARD                         # 4096 in: the allocator's alignment is kept
            assert a.tensor.data_ptr() % 64 == a.buf.data_ptr() % 64
        assert bool((a.buf[:guard.GUARD] == guard.GUARD_BYTE).all()) and bool((a.buf[guard.GUARD + a.nbytes:] == guard.GUARD_BYTE).all())
        assert bool((a.buf[guard.GUARD:guard.GUARD + a.nbytes] == guard.POISON).all())
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(z).all()) and bool(torch.isnan(w2).all()) and bool(torch.isnan(y.half()).all())
    guard.check_guards(rec.arenas)
    # writing every element the view reaches touches no guard, for the permuted NHWC view and the 1-byte-granular workspace alike
    y.fill_(1.0), z.fill_(1.0), ws.fill_(7), w2.fill_(1.0)
    guard.check_guards(rec.arenas)
    assert int((rec.arenas[0].buf[guard.GUARD:guard.GUARD + 360] == guard.POISON).sum()) == 0


def test_guarded_copy_keeps_values_and_strides():
    x = torch.randn(3, 6, 5, 3).contiguous(memory_format=torch.channels_last)[::2]              # non-dense: the gap holds the fill
    arenas = []
    g = guard.guarded_copy(x, 0xFF, arenas)
    assert torch.equal(g, x) and g.stride() == x.stride() and arenas[0].fill == 0xFF and arenas[0].nbytes == 4 * (2 * 90 + 90)
    assert bool((arenas[0].buf[:guard.GUARD] == 0xFF).all())
    guard.check_guards(arenas), guard.check_inputs_unchanged(arenas)


# ---- the case table of the GPU test is complete ------------------------------------------------------------------------------------------------------------

QUERY_SUFFIXES = ("_plan", "_supported", "_bytes", "_launches", "_gy_dtype")
QUERY_NAMES = ("rcx_abi_version", "rcx_last_error", "rcx_reload_options", "rcx_selftest_d16", "rcx_timing_begin", "rcx_timing_end", "rcx_timing_read")
# public callables of recnext_amd.ops that launch and are NOT in the case table, each with its reason
EXCLUDED = {}


def _launching_entries():
    from recnext_amd import ops
    out = {}
    for name, fn in vars(ops).items():
        if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != ops.__name__:
            continue
        called = set(re.findall(r"\b(rcx_\w+)\(", inspect.getsource(fn)))
        launches = {c for c in called if not c.endswith(QUERY_SUFFIXES) and c not in QUERY_NAMES and "timing" not in c and "selftest" not in c}
        if launches:
            out[name] = launches
    return out


def test_every_launching_entry_of_ops_is_in_the_case_table():
    from tests import test_guard_bands_gpu as t
    entries = _launching_entries()
    assert {"recconv2d_forward", "channel_mlp", "stem", "ls_la3_tiled", "unpack_recconv_grads", "linear_attention_wide_backward"} <= set(entries), sorted(entries)
    covered = {e for c in t.CASES for e in c.entry.split("+")}
    missing = sorted(set(entries) - covered - set(EXCLUDED))
    assert not missing, f"launching entries of recnext_amd.ops without a guard-band case: {missing}"
    assert not set(EXCLUDED) & covered and all(EXCLUDED.values())
    assert covered <= set(entries) | set(t.MODULE_ENTRIES), sorted(covered - set(entries))


def test_plan_family_names_every_schedule_the_library_describes():
    """Every plan head a describe function or rcx_api.hip can print maps to a family of the GPU test's required sets: a new schedule must be named there
    (and then needs a guarded case, which test_guard_bands_gpu.py::test_every_plan_family_has_a_guarded_case asserts on the GPU)."""
    from tests import test_guard_bands_gpu as t
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "recnext_amd", "csrc")
    heads = set()
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            src = open(os.path.join(csrc, name)).read()
            for fmt in re.findall(r'snprintf\(\s*(?:buf|desc)\s*,[^"]*((?:"[^"]*"\s*(?:[:?][^"]*)?)+)', src):
                heads |= set(re.findall(r'"([a-z0-9_+]+)\(', fmt))
    assert {"lanes", "plane", "cpl", "cpt", "one", "tiled", "steps+one"} <= heads, sorted(heads)
    known = {"lanes", "plane", "cpl", "cpt", "one", "tiled", "steps+one", "upadd_cpt", "%s"}          # "%s(": split / nested; upadd_cpt: the single step's plan
    assert heads <= known, f"plan heads tests/test_guard_bands_gpu.py::plan_family does not know: {sorted(heads - known)}"
    for plan, fam in [("lanes(k_recconv_lanes<7, 1, 8, 0, 4>,cb=32,ni=1,nt=256,lds=0)", "lanes7"), ("lanes(k_recconv_lanes_banded<32, 2, 16, 0, 4, 8>,cb=16", "lanes16"),
                      ("cpt(k_recconv_cpt<4, 4, 0, 128>,cb=16", "cpt56"), ("cpt(k_recconv_cpt<2, 1, 1, 512>", "cpt28"), ("cpt(k_recconv_cpt<4, 4, 0, 0, ts=16>,cb=16", "cpt64"),
                      ("cpl(k_recconv_cpl14<0, 0>,levels-1,cb=64", "cpl14"), ("cpl(k_recconv_cpl7b<0, 512>", "cpl7"), ("plane(cb=8,", "plane"), ("generic", "generic"),
                      ("split(k_down5_cpt + lanes(...) + k_upadd_cpt)", "split"), ("nested(k_down5_lanes + plane(..) + k_upadd_lanes)", "nested")]:
        assert t.plan_family(plan) == fam and fam in t.FWD_FAMILIES
    for plan, fams in [("steps", {"steps"}), ("one(k_recconv_bwd_cpl7)", {"one-cpl7"}), ("one(k_recconv_adj_cpl14,split)", {"one-cpl14", "split"}),
                       ("tiled(levels=2)+one(k_recconv_adj_cpl14)", {"tiled+one"}), ("steps+one(k_recconv_bwd_cpl14)", {"steps+one"})]:
        assert t.bwd_plan_families(plan) == fams and fams <= t.BWD_FAMILIES
    with pytest.raises(ValueError):
        t.plan_family("wave(k_new)")
    with pytest.raises(ValueError):
        t.bwd_plan_families("fused(k_new)")
