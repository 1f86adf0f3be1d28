"""Noise-map optimisation of gradient mode restated in torch: the drivers' noise_regularize / noise_normalize_
(1024_example_wing_loss_perceptual_sqz_MSE.py:32-60) for maps [1, s, s] of any float dtype, and the projection loop with
torch.optim.Adam over [latent] + noises (oracle.loss_ref.projection_gradient_ref with the maps as further parameters).  A helper of the
tests, not a test module; tests/test_noise_opt_host.py pins the regulariser on the reference's own function (tests/golden/noise_opt_reg.npz)."""
import torch

from oracle.loss_ref import get_lr_ref, noise_strength_ref


def noise_regularize_map(x):
    """One map [..., s, s]: at sides s, s/2, ... down to the first side <= 8 the squared means of x * (x rolled by one column) and
    x * (x rolled by one row), the rolls wrapping; 2 x 2 block means between the sides."""
    x = x.reshape(1, 1, x.shape[-2], x.shape[-1])
    size = x.shape[2]
    loss = 0
    while True:
        loss = loss + (x * torch.roll(x, shifts=1, dims=3)).mean().pow(2) + (x * torch.roll(x, shifts=1, dims=2)).mean().pow(2)
        if size <= 8:
            break
        x = x.reshape(1, 1, size // 2, 2, size // 2, 2).mean([3, 5])
        size //= 2
    return loss


def noise_regularize(noises):
    return sum(noise_regularize_map(n) for n in noises)


def noise_regularize_grad(x, dtype=torch.float64):
    """(value, d value / d x) of one map by autograd, evaluated in `dtype`."""
    x = x.detach().to(dtype).clone().requires_grad_(True)
    v = noise_regularize_map(x)
    v.backward()
    return v.detach(), x.grad


def noise_normalize_(noises):
    for n in noises:
        mean, std = n.mean(), n.std()                     # std: torch's default, unbiased
        n.data.add_(-mean).div_(std)


def projection_noise_ref(gen_fn, loss_fn, latent_mean, latent_std, eps_stream, noises, steps, noise_regularize_weight, lr=0.01, rampdown=0.25,
                         rampup=0.05, noise=0.05, noise_ramp=0.75, min_loss_init=100.0, adam_eps=1e-8):
    """gen_fn(latent, {name: map}) -> image; loss_fn(step, image) -> scalar tensor or None (a skipped step: nothing moves).  `noises`:
    {name: [1, s, s]} start maps.  Per step: total = loss_fn + weight * noise_regularize(maps); Adam over [latent] + maps; noise_normalize_.
    Returns dict(best_latent, best_noises, best_step, best_loss, losses, reg (the weighted regulariser per step), traj, noise_traj)."""
    latent_in = latent_mean[None].clone().requires_grad_(True)
    names = list(noises)
    maps = [noises[k].detach().clone().requires_grad_(True) for k in names]
    opt = torch.optim.Adam([latent_in] + maps, lr=lr, eps=adam_eps)
    out = dict(best_latent=None, best_noises=None, best_step=-1, best_loss=float(min_loss_init), losses=[], reg=[], traj=[], noise_traj=[])
    for i in range(steps):
        t = i / steps
        opt.param_groups[0]["lr"] = get_lr_ref(t, lr, rampdown, rampup)
        sigma = float(noise_strength_ref(t, float(latent_std), noise, noise_ramp))
        latent_n = latent_in + eps_stream[i] * sigma
        val = loss_fn(i, gen_fn(latent_n, dict(zip(names, maps))))
        if val is not None:
            reg = noise_regularize_weight * noise_regularize(maps)
            total = val + reg
            used = {k: m.detach().clone() for k, m in zip(names, maps)}
            opt.zero_grad()
            total.backward()
            opt.step()
            noise_normalize_(maps)
            num = float(total.detach())
            if num < out["best_loss"]:
                out.update(best_loss=num, best_latent=latent_n.detach().clone(), best_step=i, best_noises=used)
        out["losses"].append(None if val is None else num)
        out["reg"].append(None if val is None else float(reg.detach()))
        out["traj"].append(latent_in.detach().clone())
        out["noise_traj"].append({k: m.detach().clone() for k, m in zip(names, maps)})
    return out
