"""numpy restatements for the evolution-strategy mode (morphganformer_amd/evolution.py, csrc/evolution.hip): the recombination kernel, expression
for expression (include/mgf.h, mgf_es_recombine_f32), and the loop around it.  Shared by tests/test_evolution_host.py and
tests/test_hip_evolution.py; nothing here touches a GPU.

numpy's element-wise float64 / float32 operations round every product, quotient and sum on their own (one ufunc each, no contraction), which is
the arithmetic the kernel spells with rounding intrinsics: its results are compared bit for bit."""
import numpy as np


def log_weights(mu):
    """ln(mu + 1/2) - ln(r), r = 1..mu, normalised to sum 1 (float64)."""
    w = np.log(mu + 0.5) - np.log(np.arange(1, mu + 1, dtype=np.float64))
    return w / w.sum()


def sigma_schedule(steps, latent_std, noise=0.05, noise_ramp=0.75):
    """The drivers' sigma_i with their float32 roundings (projection.noise_schedule restated)."""
    base = np.float32(latent_std) * np.float32(noise)
    return np.array([base * np.float32(max(0, 1 - (i / steps) / noise_ramp) ** 2) for i in range(steps)], dtype=np.float32)


def elite_order(totals, s0, batch, steps_total, mu):
    """Indices j (within the generation) of the candidates that are recombined, best first: finite totals only, ascending, ties to the smaller
    j; at most mu.  None when the generation lies past the end (nothing is written at all)."""
    n = min(batch, steps_total - s0)
    if s0 < 0 or n <= 0:
        return None
    t = np.asarray(totals, dtype=np.float64)[s0:s0 + n]
    valid = np.flatnonzero(np.isfinite(t))
    return valid[np.argsort(t[valid], kind="stable")][:mu]


def es_recombine_ref(mean, cand, totals, s0, weights, mu, batch, steps_total, mean_lr=1.0):
    """-> (new mean, float32, shaped like `mean`; m, the number of candidates recombined, or None when nothing is written)."""
    mean = np.asarray(mean, dtype=np.float32)
    order = elite_order(totals, s0, batch, steps_total, mu)
    if order is None:
        return mean.copy(), None
    m = len(order)
    if m == 0:
        return mean.copy(), 0
    w = np.asarray(weights, dtype=np.float64)
    wsum = w[0]
    for r in range(1, m):
        wsum = wsum + w[r]
    c = np.asarray(cand, dtype=np.float32).reshape(batch, -1).astype(np.float64)
    S = (w[0] / wsum) * c[order[0]]
    for r in range(1, m):
        S = S + (w[r] / wsum) * c[order[r]]
    x = mean.reshape(-1).astype(np.float64)
    return (x + np.float64(mean_lr) * (S - x)).astype(np.float32).reshape(mean.shape), m


def es_loop_ref(gen_fn, loss_fn, latent_mean, latent_std, eps, steps, batch, mu, weights=None, mean_lr=1.0, noise=0.05, noise_ramp=0.75,
                min_loss_init=100.0, move=True):
    """The loop: generations of `batch` consecutive steps around a mean that moves after each (move=False: the literal loop's fixed mean).

    gen_fn(latent_n float32 [n, k, D]) -> n images; loss_fn(step, image [1, ...]) -> float, or None = "no face" (the step is skipped and its
    candidate never recombined).  eps [steps, k, D] float32.  -> dict(losses [steps] float64 with NaN for skipped steps, best_step, best_loss,
    best_latent [k, D], means: the mean after every generation, cands: every generation's candidates [batch, k, D], elites: the STEP numbers
    recombined per generation, best first, used: their count)."""
    mean = np.asarray(latent_mean, dtype=np.float32).copy()
    eps = np.asarray(eps, dtype=np.float32)
    weights = log_weights(mu) if weights is None else np.asarray(weights, dtype=np.float64)
    sigma = sigma_schedule(steps, latent_std, noise, noise_ramp)
    losses = np.full(steps, np.nan, dtype=np.float64)
    best_step, best_loss, best_latent = -1, float(min_loss_init), None
    means, cands, elites, used = [], [], [], []
    for s0 in range(0, steps, batch):
        rows = [min(s0 + j, steps - 1) for j in range(batch)]           # a ragged last generation's surplus candidates repeat the last step
        cand = np.stack([(mean + eps[s] * sigma[s]).astype(np.float32) for s in rows])
        imgs = gen_fn(cand)
        for j in range(min(batch, steps - s0)):
            val = loss_fn(s0 + j, imgs[j:j + 1])
            if val is None:
                continue
            losses[s0 + j] = float(val)
            if float(val) < best_loss:
                best_loss, best_step, best_latent = float(val), s0 + j, cand[j].copy()
        order = elite_order(losses, s0, batch, steps, mu)
        if move:
            mean, _ = es_recombine_ref(mean, cand, losses, s0, weights, mu, batch, steps, mean_lr)
        means.append(mean.copy())
        cands.append(cand)
        elites.append(s0 + order)
        used.append(len(order))
    return dict(losses=losses, best_step=best_step, best_loss=best_loss, best_latent=best_latent, means=means, cands=cands, elites=elites,
                used=np.array(used, dtype=np.int32), sigma=sigma)


def top_gaps(losses, s0, n, count=3):
    """Relative gaps between consecutive totals among the `count` best of steps s0 .. s0 + n - 1: the margin a rank comparison has."""
    t = np.sort(np.asarray(losses, dtype=np.float64)[s0:s0 + n])
    t = t[np.isfinite(t)][:count]
    return (t[1:] - t[:-1]) / np.abs(t[:-1])
