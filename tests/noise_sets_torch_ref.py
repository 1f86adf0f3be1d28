"""Sets of noise maps restated in torch (a helper of tests/test_hip_noise_sets.py and tests/test_noise_sets_host.py, not a test module):
a set is one target's maps inside a row of `set_stride` floats, map m of side sides[m] at offsets[m]; the regulariser and the normalisation
of tests/noise_opt_torch_ref.py over every map of every set, each by ONE autograd pass over the whole buffer."""
import torch

from noise_opt_torch_ref import noise_regularize_map

# sides 4 and 8: one-level maps below and at the break; 8 twice: two maps of one side; 16 and 64: two and four levels
SIDES = [4, 8, 8, 16, 64]
BIG_SIDES = [1024, 8]                  # the partial count is capped at 256 and the grid-stride loops run


def gapped_table(sides, gap=12, lead=4):
    """(offsets, extent, set_stride) with `lead` floats in front of the first map, `gap` floats between maps (multiples of 4: the maps stay
    16-byte aligned like the engine's) and a set_stride larger than the extent."""
    offsets, off = [], lead
    for s in sides:
        offsets.append(off)
        off += s * s + gap
    extent = offsets[-1] + sides[-1] ** 2
    return offsets, extent, extent + 20


def make_sets(make_map, sides, offsets, set_stride, n_sets, seed, fill=float("nan")):
    """[n_sets, set_stride] float32, every set with different data: "white" and "smooth" maps of `make_map` alternating over the maps and
    the sets; everything outside the maps is `fill`."""
    x = torch.full((n_sets, set_stride), fill, dtype=torch.float32)
    for t in range(n_sets):
        for m, (s, o) in enumerate(zip(sides, offsets)):
            x[t, o:o + s * s] = make_map(s, "smooth" if (t + m) % 2 else "white", seed + 31 * t + m).reshape(-1)
    return x


def map_of(x, t, m, sides, offsets):
    return x[t, offsets[m]:offsets[m] + sides[m] ** 2].reshape(sides[m], sides[m])


def regularize_sets(x, sides, offsets, dtype=torch.float64):
    """(values [n_sets, n_maps], gradient shaped like x with zeros outside the maps) of the regulariser of every map, evaluated in `dtype`
    by one backward pass through the sum over all of them."""
    n_sets = x.shape[0]
    xs = torch.nan_to_num(x.detach().to(dtype), nan=0.0).clone().requires_grad_(True)
    vals = [[noise_regularize_map(map_of(xs, t, m, sides, offsets)) for m in range(len(sides))] for t in range(n_sets)]
    sum(v for row in vals for v in row).backward()
    return torch.stack([torch.stack([v.detach() for v in row]) for row in vals]), xs.grad


def normalize_sets(x, sides, offsets, live, dtype=torch.float64):
    """x with every map of the sets named in `live` normalised (mean 0, unbiased std 1), evaluated in `dtype`; the rest untouched."""
    out = x.detach().to(dtype).clone()
    for t in live:
        for m in range(len(sides)):
            v = map_of(out, t, m, sides, offsets)
            v.copy_((v - v.mean()) / v.std())
    return out
