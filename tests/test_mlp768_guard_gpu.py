"""Where the (512, 768) and (384, 768) channel-mixer kernels read and write: the ragged and the padded-hidden case of tests/test_mlp768_gpu.py at each shape,
aliased (z is x: Downsample's call) and not, under the guard bands of tests/guard.py -- nothing outside y written, every element of y written, nothing
outside an operand read, no operand modified (the properties and the case construction of tests/test_guard_bands_gpu.py's channel_mlp rows)."""
import pytest
import torch

from tests import guard
from tests.test_guard_bands_gpu import BF16, cl, gen, ops, rnd
from tests.test_mlp768_gpu import SHAPES, _cases

pytestmark = pytest.mark.gpu


def _build(c, which, alias):
    n, _, hid, h, w = _cases(c)[which]
    o = ops()
    g = gen("mlp768", c, which)
    hp = o.channel_mlp_hidden(n * h * w, c, hid, BF16)
    assert hp == 768, (n, c, hid, h, w)
    wfrag, bias, hp = o.pack_channel_mlp(rnd(g, (hid, c), BF16, (2.0 / c) ** 0.5), rnd(g, (hid,), BF16, 0.3), rnd(g, (c, hid), BF16, (1.0 / hid) ** 0.5),
                                         rnd(g, (c,), BF16, 0.3), hidden_to=hp)
    z = cl(rnd(g, (n, c, h, w), BF16))
    x = z if alias else cl(rnd(g, (n, c, h, w), BF16))
    return z, x, wfrag, bias, hp


@pytest.mark.parametrize("alias", [False, True], ids=["distinct", "aliased"])
@pytest.mark.parametrize("which", ["ragged", "hidden750"])
@pytest.mark.parametrize("c", SHAPES)
def test_guard_bands(c, which, alias):
    with torch.no_grad():
        args = _build(c, which, alias)
        torch.cuda.synchronize()
        guard.run_properties(lambda z, x, wfrag, bias, hp: ops().channel_mlp(z, x, wfrag, bias, hp), args)
