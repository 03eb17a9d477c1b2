"""CPU: the plumbing the training-step operators share (recnext_amd/_trainop.py) and the module-level gates next to HipBatchNorm2d
(batchnorm.norm_fusable, batchnorm.bump).  The gates answer before any GPU call and the models' forwards leave them early for a CPU tensor, so
nothing else pins them without a GPU."""
import pytest
import torch
import torch.nn as nn

from recnext_amd import _trainop, batchnorm, bnact, dwbn, repdw

DTYPES = {4: (torch.float32,), 2: (torch.bfloat16, torch.float16)}


class _UserNorm(nn.BatchNorm2d):
    pass


def _f64_buffer():
    bn = nn.BatchNorm2d(4)
    bn.running_var = bn.running_var.double()
    return bn


@pytest.mark.parametrize("make, want", [
    (lambda: nn.BatchNorm2d(4), True),
    (lambda: batchnorm.HipBatchNorm2d(4), True),
    (lambda: nn.BatchNorm2d(4, track_running_stats=False), True),
    (lambda: batchnorm.HipBatchNorm2d(4, track_running_stats=False), True),
    (lambda: nn.BatchNorm2d(4).eval(), False),
    (lambda: batchnorm.HipBatchNorm2d(4).eval(), False),
    (lambda: nn.SyncBatchNorm(4), False),
    (lambda: _UserNorm(4), False),
    (lambda: nn.BatchNorm2d(4, affine=False), False),
    (lambda: nn.BatchNorm2d(4, momentum=None), False),
    (lambda: nn.BatchNorm2d(4).bfloat16(), False),
    (_f64_buffer, False),
], ids=["BatchNorm2d", "HipBatchNorm2d", "no-buffers", "hip-no-buffers", "eval", "hip-eval", "SyncBatchNorm", "subclass", "not-affine", "momentum-None",
        "bfloat16", "float64-buffer"])
def test_norm_fusable_truth_table(make, want):
    bn = make()
    assert bn.num_features == 4 and batchnorm.norm_fusable(bn) is want


def test_rows_routed_bounds_are_inclusive_and_a_missing_key_keeps_nothing():
    table = {("a", 2): (10, 20), ("b", 4): (7, 7)}
    for rows in (0, 1, 10, 15, 20, 10 ** 9):
        assert _trainop.rows_routed(table, ("c", 2), rows) is False and _trainop.rows_routed({}, ("a", 2), rows) is False
    assert [_trainop.rows_routed(table, ("a", 2), r) for r in (9, 10, 11, 19, 20, 21)] == [False, True, True, True, True, False]
    assert [_trainop.rows_routed(table, ("b", 4), r) for r in (6, 7, 8)] == [False, True, False]
    assert _trainop.esize(torch.float32) == 4 and _trainop.esize(torch.bfloat16) == _trainop.esize(torch.float16) == 2


def _routed_calls():
    """(id, rows -> the module's public *_routed answer) for every key of the four row-keyed tables, every dtype of the key's element size."""
    for (c, es), _ in batchnorm.ROUTED.items():
        for dt in DTYPES[es]:
            yield batchnorm.ROUTED[(c, es)], f"batchnorm-{c}-{dt}", lambda r, c=c, dt=dt: batchnorm.batch_norm_routed(r, 1, 1, c, dt)
    for (c, es), _ in repdw.ROUTED.items():
        for dt in DTYPES[es]:
            yield repdw.ROUTED[(c, es)], f"repdw-{c}-{dt}", lambda r, c=c, dt=dt: repdw.repdw_train_routed(r, 1, 1, c, dt)
    for (c, es, epi), _ in bnact.ROUTED.items():
        for dt in DTYPES[es]:
            yield bnact.ROUTED[(c, es, epi)], f"bnact-{c}-{epi}-{dt}", lambda r, c=c, dt=dt, epi=epi: bnact.bn_act_routed(r, 1, 1, c, dt, epi)
    for (c, k, s, coarse, es), _ in dwbn.ROUTED.items():
        for dt in DTYPES[es]:                                                     # a 1 x 1 plane has one output pixel at either stride: rows = N
            yield (dwbn.ROUTED[(c, k, s, coarse, es)], f"dwbn-{c}-{k}-{s}-{coarse}-{dt}",
                   lambda r, c=c, k=k, s=s, coarse=coarse, dt=dt: dwbn.dwconv_bn_train_routed(r, 1, 1, c, k, s, coarse, dt))


ROUTED_CALLS = list(_routed_calls())


@pytest.mark.parametrize("bounds, routed", [(b, f) for b, _, f in ROUTED_CALLS], ids=[i for _, i, _ in ROUTED_CALLS])
def test_every_table_row_is_kept_at_both_bounds_and_not_one_past_them(bounds, routed):
    lo, hi = bounds
    assert 1 < lo <= hi
    assert routed(lo) is True and routed(hi) is True and routed(lo - 1) is False and routed(hi + 1) is False
    assert routed((lo + hi) // 2) is True


def test_the_routed_functions_split_the_rows_over_the_plane_and_refuse_an_unknown_key():
    (c, es), (lo, hi) = next(iter(batchnorm.ROUTED.items()))
    dt = DTYPES[es][0]
    assert lo % 4 == 0 and batchnorm.batch_norm_routed(lo // 4, 2, 2, c, dt) and not batchnorm.batch_norm_routed(lo // 4 - 1, 2, 2, c, dt)
    assert not batchnorm.batch_norm_routed(lo, 1, 1, c + 1, dt) and not repdw.repdw_train_routed(lo, 1, 1, 7, dt)
    assert not bnact.bn_act_routed(lo, 1, 1, c, dt, "relu") and not dwbn.dwconv_bn_train_routed(lo, 1, 1, c, 7, 1, False, dt)
    (c, k, s, coarse, es), (lo, hi) = next((key, b) for key, b in dwbn.ROUTED.items() if key[2] == 2)
    dt = DTYPES[es][0]                                                             # stride 2: the OUTPUT rows count, ceil(H / 2) x ceil(W / 2) a plane
    assert dwbn.dwconv_bn_train_routed(hi, 2, 2, c, k, s, coarse, dt) and not dwbn.dwconv_bn_train_routed(hi, 3, 3, c, k, s, coarse, dt)
    assert lo % 4 == 0 and dwbn.dwconv_bn_train_routed(lo // 4, 3, 3, c, k, s, coarse, dt) and not dwbn.dwconv_bn_train_routed(lo // 4 - 1, 3, 3, c, k, s, coarse, dt)


def test_dense_nhwc():
    dense = _trainop.dense_nhwc
    assert batchnorm._dense_nhwc is dense
    x = torch.zeros(4, 6, 3, 5)
    assert dense(x.contiguous(memory_format=torch.channels_last)) is True
    assert dense(x) is False                                                        # NCHW-contiguous, C > 1 and H W > 1
    assert dense(x.contiguous(memory_format=torch.channels_last)[::2]) is False     # every other image: the batch stride is not H W C
    assert dense(x.contiguous(memory_format=torch.channels_last)[:, ::2]) is False
    assert dense(torch.empty_strided((1, 6, 3, 5), (12345, 1, 30, 6))) is True      # N = 1: the batch stride is never used
    assert dense(torch.empty_strided((4, 1, 3, 5), (15, 77, 5, 1))) is True         # C = 1: nor is the channel stride
    assert dense(torch.zeros(4, 1, 3, 5)) is True and dense(torch.zeros(4, 6, 1, 1)) is True
    assert dense(torch.empty_strided((1, 6, 3, 5), (12345, 15, 5, 1))) is False


def test_bump_counts_one_batch_and_hands_out_the_buffers():
    bn = nn.BatchNorm2d(4)
    bn.num_batches_tracked.fill_(41)
    before = (bn.running_mean.clone(), bn.running_var.clone())
    rm, rv = batchnorm.bump(bn)
    assert rm is bn.running_mean and rv is bn.running_var and int(bn.num_batches_tracked) == 42
    assert torch.equal(rm, before[0]) and torch.equal(rv, before[1])
    batchnorm.bump(bn)
    assert int(bn.num_batches_tracked) == 43


def test_bump_without_buffers_touches_nothing():
    bn = nn.BatchNorm2d(4, track_running_stats=False)
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    assert batchnorm.bump(bn) == (None, None)
    assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None
    assert state.keys() == bn.state_dict().keys() and all(torch.equal(v, bn.state_dict()[k]) for k, v in state.items())
