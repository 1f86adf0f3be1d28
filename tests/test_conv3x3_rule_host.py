"""conv.conv3x3_takes_winograd -- the one rule for which kernel runs a 3x3 / stride-1 / pad-1 layer -- against the expressions the call
sites spelled out before it existed, over a grid of layouts, batch sizes, widths and map sizes (no GPU: the rule reads shapes only)."""
import itertools

import pytest
import torch

from morphganformer_amd import conv as cv

CIN = 8
NS = (1, 2, 8, 32, 128, 512)
COUTS = (32, 64, 256, 512)
MAPS = ((8, 8), (16, 16), (17, 17), (18, 18), (34, 34), (63, 63), (127, 127), (256, 256), (16, 40))


def _layer(layout, cout):
    u = {"none": None, "3d": torch.empty(16, CIN, cout), "4d": torch.empty(16, CIN // 4, cout, 4)}[layout]
    return cv.Conv3x3(cv.PackedConv(None, None, cout, CIN, 3, 3, cv.round_up(cout, 32)), u)


@pytest.mark.parametrize("form", [2, 3])
def test_the_rule_chooses_what_the_call_sites_chose(form, monkeypatch):
    monkeypatch.setattr(cv, "WINOGRAD_FORM", form)
    seen = {(layout, took): 0 for layout in ("none", "3d", "4d") for took in (False, True)}
    for layout, n, cout, (h, w) in itertools.product(("none", "3d", "4d"), NS, COUTS, MAPS):
        layer = _layer(layout, cout)
        assert (layer.cin, layer.cout) == (CIN, cout)
        u = layer.u
        took = cv.conv3x3_takes_winograd(layer, n, h, w)
        assert isinstance(took, bool)
        seen[(layout, took)] += 1
        where = (form, layout, n, cout, h, w)
        # the generator and its gradient: planes in the layout winograd_pack gives the layer's one (square) map size -- 3-D at 16^2, 4-D above
        if layout == "none" or (layout == "3d" and (h, w) == (16, 16)) or (layout == "4d" and min(h, w) > 16):
            assert took == (u is not None and cv.winograd_fills_chip(n, cout, h, w)), where
        if layout == "4d":
            # the LPIPS backbones: forms-2/3 planes at every map size, guarded
            assert took == (min(h, w) > 16 and cv.winograd_fills_chip(n, cout, h, w)), where
            if min(h, w) <= 16:
                # ... and the sites that had no guard (FaceNet, the expand-3x3 data gradient) applied form 1's count to forms-2/3 planes
                # here: the one rule says tap list
                assert took is False, where
        if layout == "3d" and min(h, w) > 16:
            assert took is False, where                                # form 1's planes serve the 16 px maps only
    assert seen[("none", True)] == 0 and seen[("none", False)] > 0
    assert all(seen[(layout, took)] > 0 for layout in ("3d", "4d") for took in (False, True)), seen


def test_the_rule_reads_winograd_fills_chip_at_call_time(monkeypatch):
    layer = _layer("4d", 32)
    assert not cv.conv3x3_takes_winograd(layer, 1, 18, 18)
    monkeypatch.setattr(cv, "winograd_fills_chip", lambda n, cout, h, w: True)
    assert cv.conv3x3_takes_winograd(layer, 1, 18, 18)
    assert not cv.conv3x3_takes_winograd(layer, 1, 16, 16) and not cv.conv3x3_takes_winograd(_layer("none", 32), 1, 18, 18)
