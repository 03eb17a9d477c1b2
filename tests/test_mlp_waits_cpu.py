"""The pinned hidden step of the channel mixer (rcx_mlp.hip hidden_tile_pinned) keeps its LDS requests in flight: in the listing the build leaves
(recnext_amd/csrc/_obj/rcx_mlp.s, read by tools/check_mlp_waits.py) the hidden-step loop of every kernel that takes the pinned form (k_channel_mlp_pair) has at most three full drains
(s_waitcnt lgkmcnt(0)) between its first and last product -- one per product chain for its tail and one for the b1 / GELU hand-off.  A condition of the design,
not a measurement: a compiler or flag change that regroups the requests fails here before it costs time on a GPU."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTING = os.path.join(ROOT, "recnext_amd", "csrc", "_obj", "rcx_mlp.s")
PINNED = {"k_channel_mlp_pair": (32, 1)}      # the kernels that take the pinned form -> (products, hidden steps) of an iteration of their hidden-step loop


def _tool():
    spec = importlib.util.spec_from_file_location("check_mlp_waits", os.path.join(ROOT, "tools", "check_mlp_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_wait_report_reads_a_listing(tmp_path):
    """the tool on a listing made here: a loop of four products, five reads, one full drain between the first and the last product"""
    body = ["_ZN3rcx3mlp18k_channel_mlp_pairILi1ELi2ELi1ELb1EEEvPKt: ; @x", ".LBB0_1:"]
    body += ["\tds_read_b128 v[0:3], v9", "\tds_read_b128 v[4:7], v9 offset:1024", "\ts_waitcnt lgkmcnt(1)", "\tv_mfma_f32_32x32x16_bf16 v[16:31], v[0:3], v[8:11], 0"]
    body += ["\tds_read_b128 v[0:3], v9 offset:2048", "\ts_waitcnt lgkmcnt(1)", "\tv_mfma_f32_32x32x16_bf16 v[16:31], v[4:7], v[8:11], v[16:31]"]
    body += ["\tds_read_b128 v[4:7], v9 offset:3072", "\tds_read_b128 v[12:15], v9 offset:4096", "\ts_waitcnt lgkmcnt(2)", "\tv_mfma_f32_32x32x16_bf16 v[16:31], v[0:3], v[8:11], v[16:31]"]
    body += ["\ts_waitcnt lgkmcnt(0)", "\tv_mfma_f32_32x32x16_bf16 v[16:31], v[4:7], v[8:11], v[16:31]", "\ts_cbranch_scc1 .LBB0_1", "\ts_endpgm"]
    p = tmp_path / "t.s"
    p.write_text("\n".join(body) + "\n")
    rows = _tool().report(str(p))
    assert len(rows) == 1
    r = rows[0]
    assert (r["kernel"], r["template"]) == ("k_channel_mlp_pair", [1, 2, 1])
    assert (r["products_per_step"] * r["steps_per_iteration"], r["ds_reads_per_step"] * r["steps_per_iteration"]) == (4, 5)
    assert r["full_drains_per_step"] * r["steps_per_iteration"] == 1 and r["min_in_flight"] == 0


@pytest.mark.skipif(not os.path.exists(LISTING), reason="no listing: recnext_amd/csrc/_obj/rcx_mlp.s is left by the library's build (make -C recnext_amd/csrc all)")
def test_pinned_hidden_steps_have_at_most_three_full_drains():
    rows = [r for r in _tool().report(LISTING) if r["kernel"] in PINNED]
    assert {r["kernel"] for r in rows} == set(PINNED), "a pinned kernel's hidden-step loop was not found in the listing"
    for r in rows:
        prods, steps = PINNED[r["kernel"]]
        print(f"\n{r['kernel']}<{r['template']}>: {r['full_drains_per_step']} full drains, {r['ds_reads_per_step']} reads, {r['products_per_step']} products a hidden step; "
              f"least left in flight {r['min_in_flight']}")
        assert r["products_per_step"] == prods and r["steps_per_iteration"] == steps
        assert r["full_drains_per_step"] <= 3
