"""CPU: the masked float64 restatement of tests/embed_masked_ref.py is the oracle's own network, and the per-boundary gate built on it
(tests/test_hip_embed_blocks.py) rejects the confined faults that the bulk gates of test_hip_embed.py let through."""
import functools

import pytest
import torch

import embed_masked_ref as mr
from morphganformer_amd import facenet, iresnet
from oracle.embed_ref import inception_resnet_v1_ref, iresnet_ref

CASES = {"facenet": ("facenet", lambda: facenet.random_state(9), (2, 3, 99, 131)),
         "iresnet18": ("iresnet18", lambda: iresnet.random_state(18, 3), (2, 3, 112, 112))}


def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 2 - 1, torch.randn(shape[0], 512, generator=g)


@functools.lru_cache(maxsize=None)
def _clean(name):
    """Per network: the float32 restatement's own masks, and under them the float64 reference and the float32 gradient (the clean `got`)."""
    net, make, shape = CASES[name]
    sd = make()
    img, demb = _inputs(shape, 5)
    _, rec32, _ = mr.free_run(net, sd, img, torch.float32, keep_pre=False)
    _, ref64 = mr.masked_gradients(net, sd, img, demb, rec32.masks, rec32.pool_idx, torch.float64)
    _, got32 = mr.masked_gradients(net, sd, img, demb, rec32.masks, rec32.pool_idx, torch.float32)
    return dict(net=net, sd=sd, img=img, demb=demb, rec32=rec32, ref64=ref64, got32=got32)


@pytest.mark.parametrize("name", list(CASES))
def test_masked_restatement_under_its_own_masks_is_the_free_network(name):
    """(a) Fed the float64 run's own masks and pool indices, the hook reproduces the oracle's free gradient to 1e-12 -- at the image against the
    oracle called WITHOUT a hook, at every boundary against the recording run -- and the same embedding."""
    net, make, shape = CASES[name]
    sd = make()
    img, demb = _inputs(shape, 6)
    sd64 = mr.state(sd, torch.float64)
    x = img.double().requires_grad_(True)
    if net == "facenet":
        emb = inception_resnet_v1_ref(sd64, x)
    else:
        emb = iresnet_ref(sd64, x, 18)
    (plain,) = torch.autograd.grad((emb * demb.double()).sum(), x)
    emb_free, rec, free = mr.free_run(net, sd, img, torch.float64, demb)
    assert torch.equal(emb_free, emb.detach())
    emb_m, masked = mr.masked_gradients(net, sd, img, demb, rec.masks, rec.pool_idx, torch.float64)
    assert float((emb_m - emb_free).abs().max()) <= 1e-12 * float(emb_free.abs().max())
    assert float((masked["img"] - plain).abs().max()) <= 1e-12 * float(plain.abs().max())
    for b in mr.boundaries(net):
        assert float((masked[b] - free[b]).abs().max()) <= 1e-12 * float(free[b].abs().max()), b
    assert mr.check_masks(rec.masks, rec.pool_idx, rec)[0] == 0


@pytest.mark.parametrize("name", list(CASES))
def test_clean_float32_passes_everywhere(name):
    clean = _clean(name)
    rows = mr.gate_rows(clean["net"], clean["got32"], clean["ref64"], clean["got32"])
    mr.check_gate(rows, clean["net"] + " float32 restatement, clean")
    assert not mr.failing(rows)
    # the masks of the float32 run against the free float64 run: few, and only units at their kink
    _, rec64, _ = mr.free_run(clean["net"], clean["sd"], clean["img"], torch.float64)
    flips, total = mr.check_masks(clean["rec32"].masks, clean["rec32"].pool_idx, rec64)
    print(f"{clean['net']}: float32 and float64 disagree on {flips} of {total} units")


# (network, layer, fault, the boundary directly in front of the layer)
FAULTS = [("facenet", "conv2d_1a", "last_row", "img"),
          ("facenet", "conv2d_4b", "last_row", "in:conv2d_4b"),
          ("facenet", "conv2d_4b", "last_col", "in:conv2d_4b"),
          ("facenet", "conv2d_2b", "ring", "in:conv2d_2b"),
          ("facenet", "repeat_1.1.branch1.1", "last_channel", "in:repeat_1.1"),
          ("facenet", "repeat_2.4.branch1.1", "no_mask", "in:repeat_2.4"),
          ("iresnet18", "layer2.0.prelu", "roll_slope", "in:layer2.0")]


@pytest.mark.parametrize("net,layer,kind,front", FAULTS, ids=[f"{f[1]}-{f[2]}" for f in FAULTS])
def test_the_gate_rejects_a_confined_fault(net, layer, kind, front):
    """(b) One fault in the backward of one layer of the float32 restatement: the gate fails at the boundary directly in front of the layer and at
    the image, and at no boundary behind the layer (closer to the embedding).  For the three last-row / last-column faults at 99x131 the median
    and rms of the image gradient's error are printed beside the bulk gate of test_facenet_gradient_matches_autograd (2e-5, 2e-3)."""
    clean = _clean(net)
    _, got = mr.masked_gradients(net, clean["sd"], clean["img"], clean["demb"], clean["rec32"].masks, clean["rec32"].pool_idx, torch.float32,
                                 faults={layer: kind})
    rows = mr.gate_rows(net, got, clean["ref64"], clean["got32"])
    bad = mr.failing(rows)
    names = mr.boundaries(net)
    img_row = rows[-1]
    print(f"{layer} {kind}: fails at {len(bad)} boundaries from {bad[0] if bad else None}; image: max {img_row['err']:.3e} median {img_row['median']:.3e} "
          f"rms {img_row['rms']:.3e} (bound {img_row['bound']:.3e})")
    assert front in bad and "img" in bad
    assert bad[0] == front and all(names.index(b) >= names.index(front) for b in bad)
    with pytest.raises(AssertionError, match="the deepest is " + front.replace(".", r"\.")):
        mr.check_gate(rows, f"{layer} {kind}")
    if kind in ("last_row", "last_col"):
        # the record of why this gate exists (printed, not asserted: the figures move with the input; on test_facenet_gradient_matches_autograd's
        # own seeds they were rms 1.6e-4 / 1.82e-3 / 1.13e-3 and median <= 1.8e-7, all inside that test's gate)
        print(f"    the bulk gate of test_facenet_gradient_matches_autograd asks median < 2e-5 and rms < 2e-3: median {img_row['median']:.3e} "
              f"{'passes' if img_row['median'] < 2e-5 else 'fails'}, rms {img_row['rms']:.3e} {'passes' if img_row['rms'] < 2e-3 else 'fails'}")


def test_first_maximum_rule_on_ties():
    """(c) A window of equal values and windows of exact zeros take their FIRST element in row-major order; a tie between two maxima takes the
    earlier; a negative element loses to the zeros before and after it."""
    x = torch.zeros(1, 2, 5, 7, dtype=torch.float64)
    x[0, 0] = 3.0                                                      # every window equal: its top-left element, (2 oy, 2 ox)
    x[0, 1, 1, 3] = 2.0                                                # channel 1: zeros, two equal maxima that window (0, 1) sees both ...
    x[0, 1, 2, 4] = 2.0
    x[0, 1, 4, 0] = -1.0
    idx = mr.first_max_indices(x)
    assert tuple(idx.shape) == (1, 2, 2, 3)
    w = 7
    assert idx[0, 0].tolist() == [[0, 2, 4], [2 * w, 2 * w + 2, 2 * w + 4]]
    # channel 1, window (oy, ox) = rows 2 oy .. 2 oy + 2, columns 2 ox .. 2 ox + 2:
    #   (0,0) all zeros -> (0,0);  (0,1) holds both 2.0 -> the earlier, (1,3);  (0,2) -> (2,4);
    #   (1,0) zeros and the -1 -> its first zero, (2,0);  (1,1) -> (2,4);  (1,2) -> (2,4), its own first element
    assert idx[0, 1].tolist() == [[0, 1 * w + 3, 2 * w + 4], [2 * w, 2 * w + 4, 2 * w + 4]]
    assert torch.equal(x.reshape(1, 2, -1).gather(2, idx.reshape(1, 2, -1)).reshape(idx.shape), torch.nn.functional.max_pool2d(x, 3, stride=2))
