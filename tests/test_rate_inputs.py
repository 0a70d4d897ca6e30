"""GPU: the input contract the rate calls share (rate._curve_inputs) on device-resident tensors -- int64 grain indices, an e8 map
of twice the e16 map's size -- is checked by every one of them before anything is launched.  One 16x16-pixel image: h16 = w16 = 1.
The codec handed in is None: a call that got past the check would fail on it, not launch on inputs the kernels do not take."""
import pytest
import torch

import control_gic_amd as cg

pytestmark = pytest.mark.gpu
DEV = "cuda"

CALLS = {
    "rate_table": lambda g: cg.rate_table(None, *g, [(0.1, 0.4)]),
    "rate_curve": lambda g: cg.rate_curve(None, *g, 0.1),
    "route_to_bpp": lambda g: cg.route_to_bpp(None, *g, 0.1, target_bpp=1.0),
    "rate_curve_tiled": lambda g: cg.rate_curve_tiled(None, [(*g, [0])], 0.1),
}


def _group(ind_dtype=torch.int64, e8_shape=(1, 2, 2)):
    inds = [torch.zeros((1, s, s), dtype=ind_dtype, device=DEV) for s in (1, 2, 4)]
    return (*inds, torch.zeros((1, 1, 1), device=DEV), torch.zeros(e8_shape, device=DEV))


@pytest.mark.parametrize("bad", [dict(ind_dtype=torch.int32), dict(e8_shape=(1, 2, 3))], ids=["int32 indices", "e8 of the wrong shape"])
@pytest.mark.parametrize("name", list(CALLS))
def test_every_rate_call_checks_its_inputs_before_any_launch(name, bad):
    with pytest.raises(ValueError):
        CALLS[name](_group(**bad))
