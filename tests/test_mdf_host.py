"""The MDF objective's host side (morphganformer_amd/mdf.py), no GPU: the restricted reader of the Ds_*.pth weight files, the float64
BatchNorm folding, and a float64 restatement of the reference's MDFLoss against tests/golden/mdf_tiny.npz (tools/make_mdf_golden.py)."""
import hashlib
import io
import os
import pickle
import sys
import types
import zipfile

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from morphganformer_amd import mdf  # noqa: E402
from morphganformer_amd._lib import MgfError  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "mdf_tiny.npz")


def mdf_taps64(sd, x):
    """float64 restatement of one discriminator's taps (conv -> eval BatchNorm -> LeakyReLU(0.2), valid 3x3 convs)."""
    dev = x.device
    g = lambda k: torch.as_tensor(sd[k], dtype=torch.float64, device=dev)
    taps = []
    for i, (c, nrm) in enumerate(zip(mdf._CONVS, mdf._NORMS)):
        x = F.conv2d(x, g(c + ".weight"), g(c + ".bias"))
        x = (x - g(nrm + ".running_mean")[:, None, None]) / torch.sqrt(g(nrm + ".running_var")[:, None, None] + 1e-5)
        x = F.leaky_relu(x * g(nrm + ".weight")[:, None, None] + g(nrm + ".bias")[:, None, None], 0.2)
        if i == 0 or i == len(mdf._CONVS) - 1:
            taps.append(x)
    return taps + [F.conv2d(x, g("tail.weight"), g("tail.bias"))]


def mdf_loss64(Ds, target, cand, num_scales=8, asc=1):
    """[n, num_scales, 3] per-tap means and [n] losses (mdfloss.py:16-47 per candidate) in float64."""
    t = torch.as_tensor(np.asarray(target), dtype=torch.float64)
    y = torch.as_tensor(np.asarray(cand), dtype=torch.float64)
    out = np.zeros((y.shape[0], num_scales, 3))
    for i in range(num_scales):
        sd = Ds[i if asc else len(Ds) - 1 - i]
        tx, ty = mdf_taps64(sd, t), mdf_taps64(sd, y)
        for k in range(3):
            out[:, i, k] = ((ty[k] - tx[k]) ** 2).mean(dim=(1, 2, 3)).numpy()
    return out, out.sum(axis=(1, 2))


def _digest(Ds):
    h = hashlib.sha256()
    for sd in Ds:
        for k in sorted(sd):
            h.update(k.encode() + np.ascontiguousarray(sd[k], dtype=np.float32).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("case", ["asc8", "asc5", "desc9"])
def test_float64_restatement_reproduces_reference_fixture(case):
    g = np.load(GOLDEN)
    seed, nd, scales, asc = (int(v) for v in g[f"{case}_cfg"])
    nfc = (32,) * 4 + (64,) * 4 + ((128,) if nd == 9 else ())
    Ds = mdf.random_discriminators(seed, nfc)
    assert _digest(Ds) == str(g[f"{case}_digest"]), "random_discriminators no longer draws the fixture's weights"
    taps, loss = mdf_loss64(Ds, g["target"], g["candidates"], scales, asc)
    assert np.abs(taps - g[f"{case}_taps"]).max() <= 1e-5 * np.abs(g[f"{case}_taps"]).max()
    assert np.allclose(loss, g[f"{case}_loss"], rtol=1e-5, atol=0)
    assert abs(loss.mean() - float(g[f"{case}_mean"])) <= 1e-5 * abs(float(g[f"{case}_mean"]))


# ------------------------------------------------------------------------------------------------------------ weight files
class _ConvBlock(nn.Sequential):
    def __init__(self, cin, cout):
        super().__init__()
        self.add_module("conv", nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=0))
        self.add_module("norm", nn.BatchNorm2d(cout))
        self.add_module("LeakyRelu", nn.LeakyReLU(0.2, inplace=True))


class _WDisc(nn.Module):
    def __init__(self, N):
        super().__init__()
        self.head = _ConvBlock(3, N)
        self.body = nn.Sequential()
        for i in range(3):
            self.body.add_module(f"block{i + 1}", _ConvBlock(N, N))
        self.tail = nn.Conv2d(N, 1, kernel_size=3, stride=1, padding=0)


@pytest.fixture
def singan_modules():
    """Throwaway `SinGAN.models` classes, registered only while the file is written (the reader must not need them)."""
    pkg, mod = types.ModuleType("SinGAN"), types.ModuleType("SinGAN.models")
    for cls, name in ((_ConvBlock, "ConvBlock"), (_WDisc, "WDiscriminator")):
        cls.__module__, cls.__qualname__, cls.__name__ = "SinGAN.models", name, name
        setattr(mod, name, cls)
    pkg.models = mod
    sys.modules["SinGAN"], sys.modules["SinGAN.models"] = pkg, mod
    yield
    sys.modules.pop("SinGAN", None)
    sys.modules.pop("SinGAN.models", None)


def _seeded_modules(nfc=(32, 64)):
    Ds = []
    for sd in mdf.random_discriminators(5, nfc):
        D = _WDisc(sd["head.conv.weight"].shape[0])
        D.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        Ds.append(D.eval())
    return Ds


@pytest.mark.parametrize("zip_format", [False, True])
def test_reader_reads_module_lists_without_importing_them(tmp_path, singan_modules, zip_format):
    Ds = _seeded_modules()
    path = str(tmp_path / "Ds.pth")
    torch.save(Ds, path, _use_new_zipfile_serialization=zip_format)
    assert zipfile.is_zipfile(path) == zip_format
    sys.modules.pop("SinGAN", None)
    sys.modules.pop("SinGAN.models", None)
    got = mdf.load_discriminators(path)
    assert "SinGAN" not in sys.modules and "SinGAN.models" not in sys.modules
    assert len(got) == len(Ds)
    for D, sd in zip(Ds, got):
        ref = {k: v for k, v in D.state_dict().items() if not k.endswith("num_batches_tracked")}
        assert set(ref) == set(k for k in sd if k != "eps")
        for k, v in ref.items():
            assert torch.equal(sd[k], v.float()), k
        assert sd["eps"] == 1e-5


def test_reader_accepts_state_dict_lists(tmp_path):
    sds = mdf.random_discriminators(2, (32,))
    path = str(tmp_path / "sd.pth")
    torch.save([{k: torch.from_numpy(v) for k, v in sd.items()} for sd in sds], path)
    got = mdf.load_discriminators(path)
    assert all(np.array_equal(got[0][k].numpy(), v) for k, v in sds[0].items())


class _Evil:
    def __reduce__(self):
        return (os.system, ("touch should_not_exist",))


@pytest.mark.parametrize("zip_format", [False, True])
def test_reader_refuses_foreign_globals_without_running_them(tmp_path, zip_format, monkeypatch):
    monkeypatch.chdir(tmp_path)
    path = str(tmp_path / "evil.pth")
    torch.save([_Evil()], path, _use_new_zipfile_serialization=zip_format)
    with pytest.raises(MgfError, match="refusing"):
        mdf.load_discriminators(path)
    assert not (tmp_path / "should_not_exist").exists()


def test_reader_checks_the_architecture(tmp_path, singan_modules):
    D = _seeded_modules((32,))[0]
    D.body.block2.conv.padding = (1, 1)
    path = str(tmp_path / "pad.pth")
    torch.save([D], path, _use_new_zipfile_serialization=False)
    with pytest.raises(MgfError, match="padding"):
        mdf.load_discriminators(path)
    D = _seeded_modules((32,))[0]
    D.train()
    torch.save([D], path, _use_new_zipfile_serialization=False)
    with pytest.raises(MgfError, match="training"):
        mdf.load_discriminators(path)
    bad = mdf.random_discriminators(0, (48,))
    with pytest.raises(MgfError, match="width"):
        mdf.check_state(bad[0])


def test_bn_folding_matches_eval_module_in_float64():
    sd = mdf.random_discriminators(3, (32,))[0]
    layers = mdf.fold_bn(sd)
    x = torch.randn(2, 3, 12, 12, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    for i, (c, nrm) in enumerate(zip(mdf._CONVS, mdf._NORMS)):
        cin = 3 if i == 0 else 32
        conv, bn = nn.Conv2d(cin, 32, 3).double(), nn.BatchNorm2d(32).double().eval()
        conv.load_state_dict({"weight": torch.from_numpy(sd[c + ".weight"]), "bias": torch.from_numpy(sd[c + ".bias"])})
        bn.load_state_dict({k: torch.from_numpy(sd[f"{nrm}.{k}"]) for k in ("weight", "bias", "running_mean", "running_var")}, strict=False)
        xi = x if i == 0 else torch.randn(2, 32, 12, 12, dtype=torch.float64)
        with torch.no_grad():
            ref = bn(conv(xi))
        got = F.conv2d(xi, torch.from_numpy(layers[i][0]), torch.from_numpy(layers[i][1]))
        assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


def test_real_weight_file_layout_if_present():
    """The published Ds_*.pth are legacy pickles of 8 / 9 modules (N = 32 x 4, 64 x 4[, 128]); only checked where such a file is
    named by MGF_MDF_WEIGHTS (no file of the reference is part of this repository)."""
    path = os.environ.get("MGF_MDF_WEIGHTS")
    if not path:
        Ds = mdf.random_discriminators()
        assert [sd["head.conv.weight"].shape[0] for sd in Ds] == [32] * 4 + [64] * 4
        return
    Ds = mdf.load_discriminators(path)
    assert [int(sd["head.conv.weight"].shape[0]) for sd in Ds][:8] == [32] * 4 + [64] * 4
