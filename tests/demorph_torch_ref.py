"""The coupled de-morphing loop as torch autograd + torch.optim.Adam([p_A, p_B]) on the CPU, on the lines of
oracle.loss_ref.projection_gradient_ref -- the oracle of demorph.DemorphEngine (tests/test_hip_demorph.py).  A helper, not a test."""
import torch

from oracle.loss_ref import get_lr_ref, noise_strength_ref


def demorph_ref(gen_fn, loss_fn, start_a, start_b, latent_std, eps_stream, steps, alpha, row_weight=(1.0, 1.0), lr=0.01, rampdown=0.25,
                rampup=0.05, noise=0.05, noise_ramp=0.75, min_loss_init=100.0, adam_eps=1e-8, weight_decay=0.0):
    """gen_fn(latents [n, ...]) -> images [n, ...];  loss_fn(step, row, image [1, ...]) -> scalar tensor, or None: the step is skipped and
    nothing moves.  eps_stream [steps, 2, ...]: row 0 perturbs p_A, row 1 p_B.  Per step

        n_A, n_B = p_A + eps[i, 0] sigma_i, p_B + eps[i, 1] sigma_i
        rows     = [float32(1 - alpha) n_A + float32(alpha) n_B,  n_A]        (merge_morph's float32 blend)
        total    = row_weight[0] loss_fn(i, 0, G(rows[0])) + row_weight[1] loss_fn(i, 1, G(rows[1]))

    and one Adam step over both parameters.  Returns dict(traj_a, traj_b: the parameters after every step; losses: the joint totals (None =
    skipped); row_losses [2][steps]; best_step, best_loss, best_a, best_b: the perturbed pair of the best step)."""
    p_a = start_a.detach().clone().requires_grad_(True)
    p_b = start_b.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([p_a, p_b], lr=lr, eps=adam_eps, weight_decay=weight_decay)
    c_a, c_b = torch.tensor(1.0 - alpha, dtype=torch.float32), torch.tensor(alpha, dtype=torch.float32)
    out = dict(traj_a=[], traj_b=[], losses=[], row_losses=[[], []], best_step=-1, best_loss=float(min_loss_init), best_a=None, best_b=None)
    for i in range(steps):
        t = i / steps
        opt.param_groups[0]["lr"] = get_lr_ref(t, lr, rampdown, rampup)
        sigma = float(noise_strength_ref(t, float(latent_std), noise, noise_ramp))
        n_a, n_b = p_a + eps_stream[i, 0] * sigma, p_b + eps_stream[i, 1] * sigma
        rows = torch.stack([c_a * n_a + c_b * n_b, n_a])
        img = gen_fn(rows)
        vals = [loss_fn(i, b, img[b:b + 1]) for b in range(2)]
        if vals[0] is None or vals[1] is None:
            out["losses"].append(None)
            for b in range(2):
                out["row_losses"][b].append(None)
        else:
            total = row_weight[0] * vals[0] + row_weight[1] * vals[1]
            opt.zero_grad()
            total.backward()
            opt.step()
            num = float(total.detach())
            out["losses"].append(num)
            for b in range(2):
                out["row_losses"][b].append(float(vals[b].detach()))
            if num < out["best_loss"]:
                out.update(best_loss=num, best_step=i, best_a=n_a.detach().clone(), best_b=n_b.detach().clone())
        out["traj_a"].append(p_a.detach().clone())
        out["traj_b"].append(p_b.detach().clone())
    return out
