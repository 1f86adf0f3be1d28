"""Cases, seeded inputs and float64 references shared by tests/test_hip_style_demod.py (GPU) and tests/test_style_demod_host.py (CPU): the
styles s and demodulation coefficients d of a modulated layer (csrc/latent_prep.hip) and their adjoint (csrc/backward.hip), in every
launch form.

The formulas are the ones include/mgf.h states for mgf_style_job, mgf_demod_f32 / mgf_demod_bwd_f32 and mgf_style_bwd_job:
    s[n,i]      = ((sum_k wg[n,k] aff_w[i,k]) aff_gain + aff_b[i]) style_gain,      wg = ws[n * ws_stride_n + w_offset ...]
    d[n,o]      = rsqrt(sum_i wsq[o,i] s[n,i]^2 + 1e-8)
    ds[n,i]     = sum_chunks ds_part[n,i,:] - s[n,i] sum_o (sum_chunks dc_part[n,o,:]) d[n,o]^2 wsq[o,i]       (second term: demodulation)
    dwg[n,k]    = aff_gain style_gain sum_i ds[n,i] aff_w[i,k]
    ds_op[n,i]  = -s[n,i] sum_o dd[n,o] d[n,o]^3 wsq[o,i]
tests/test_style_demod_host.py ties the last three to torch autograd of the first two.  Nothing here is derived from a kernel.

Every operand is drawn in float64 and ROUNDED TO FLOAT32 (kept as float64), so the kernels read exactly the numbers the references use.
wsq is sum_taps w^2 of a random 3x3 weight scaled by 1 / sqrt(9 cin) (the layer's weight gain): non-negative, about 1 / cin.

Sample roles.  NORMAL: latents ~ N(0, 1).  SMALL: the latent row times 1e-3 -- in a job with aff_b = 0 the styles are about 1e-3,
sum wsq s^2 about 1e-6 and the 1e-8 inside the rsqrt is 1 % of it.  ZERO: the latent row 0 -- with aff_b = 0, s = 0 and d = 1e4 exactly.
A case with n >= 3 samples has sample 1 SMALL and sample n - 1 ZERO, and at least one demodulated job with aff_b = 0.
"""
import math

import torch

DOT_TOL = 1e-5                        # the project's gate for float32 dot-product kernels (tests/test_hip_latent_counts.py)
EPS = 1e-8
WDIM = 32
SLOTS = 3                             # ws [n, SLOTS, wdim]: job j reads slot 1 + j % 2, slot 0 is never a job's
NORMAL, SMALL, ZERO = "normal", "small", "zero"
F64 = torch.float64


def f32r(t):
    """Round to float32, keep as float64: what a float32 device buffer holds."""
    return t.to(torch.float32).to(F64)


def roles_for(n):
    r = [NORMAL] * n
    if n >= 3:
        r[1], r[n - 1] = SMALL, ZERO
    return r


def _scale_rows(x, roles):
    """x [n, ...]: the SMALL rows times 1e-3, the ZERO rows 0."""
    for i, role in enumerate(roles):
        if role == SMALL:
            x[i] *= 1e-3
        elif role == ZERO:
            x[i] = 0.0
    return x


def make_wsq(cout, cin):
    w = torch.randn(cout, cin, 3, 3, dtype=F64) / math.sqrt(9 * cin)
    return f32r(w.square().sum(dim=(2, 3)))


# ---------------------------------------------------------------------------------------------- forward: styles + demodulation
# job: (cin, cout, demod, bias) -- bias False: aff_b = 0 (the job in which the SMALL / ZERO samples have small / zero styles)
_JOBS_AB = ((4, 3, True, False), (20, 100, True, False), (48, 32, False, True), (64, 64, True, True))
# id: (n, jobs, max_cin handed to mgf_style_demod_multi)
FORWARD_CASES = {
    "A0": (1, _JOBS_AB, 0),                                            # per-sample form (n == 1); cout 3 < 16 grid blocks, cin % 64 != 0
    "A64": (1, _JOBS_AB, 64),
    "B64": (3, _JOBS_AB, 64),                                          # batched form
    "B0": (3, _JOBS_AB, 0),                                            # per-sample form (max_cin unknown)
    "C": (32, ((512, 8, True, False), (20, 5, True, True), (24, 3, False, True)), 512),          # batched, exactly 64 KiB of dynamic LDS
    "D": (17, ((1024, 8, True, False), (48, 70, True, False), (24, 3, False, True)), 1024),      # batched, 68 KiB: the raised LDS limit
    "E": (32, ((1024, 6, True, False), (24, 3, False, True)), 1024),                             # batched, exactly 128 KiB
    "F": (33, ((64, 16, True, False), (24, 3, False, True)), 64),                                # n > 32: per-sample form
    "G": (17, ((2048, 6, True, False), (24, 3, False, True)), 2048),                             # > 128 KiB: per-sample form, cin at the styles' LDS cap
}
BATCHED_FORWARD = ("B64", "C", "D", "E")                              # the ids that reach style_demod_batched_kernel
SINGLE_JOB_CASES = [(n, cin, cout) for n in (1, 3) for (cin, cout) in ((20, 100), (2048, 6))]


def style_jobs(n, jobs, seed, wdim=WDIM):
    """-> ws [n, SLOTS, wdim], ws_stride_n, [job dict]: seeded float32-representable operands of one styles + demodulation launch."""
    torch.manual_seed(seed)
    roles = roles_for(n)
    ws = torch.randn(n, SLOTS, wdim, dtype=F64)
    _scale_rows(ws[:, 1:], roles)                                      # (slot 0 stays N(0, 1): a w_offset of 0 reads plausible numbers)
    out = []
    for j, (cin, cout, demod, bias) in enumerate(jobs):
        slot = 1 + j % 2
        out.append(dict(cin=cin, cout=cout, demod=demod, w_offset=slot * wdim, slot=slot, aff_w=f32r(torch.randn(cin, wdim, dtype=F64)),
                        aff_b=f32r(1 + 0.5 * torch.randn(cin, dtype=F64)) if bias else torch.zeros(cin, dtype=F64),
                        wsq=make_wsq(cout, cin) if demod else None, aff_gain=float(f32r(torch.tensor(1.0 / math.sqrt(wdim)))),
                        style_gain=1.25 if demod else float(f32r(torch.tensor(1.0 / math.sqrt(cin))))))
    return f32r(ws), SLOTS * wdim, out


def forward_case(cid):
    n, jobs, max_cin = FORWARD_CASES[cid]
    return style_jobs(n, jobs, 9000 + 17 * n + sum(j[0] for j in jobs))           # (A0 / A64 and B64 / B0 share their operands)


def single_job_case(n, cin, cout):
    ws, stride, jobs = style_jobs(n, ((cin, cout, True, False),), 9500 + 7 * n + cin)
    return ws, stride, jobs[0]


def styles_ref(ws, job):
    """-> s [n, cin], and the sum of the absolute values of the terms of every element (what its float32 error scales with)."""
    wg = ws[:, job["slot"]]
    s = (wg @ job["aff_w"].T * job["aff_gain"] + job["aff_b"][None]) * job["style_gain"]
    sabs = (wg.abs() @ job["aff_w"].abs().T * job["aff_gain"] + job["aff_b"].abs()[None]) * abs(job["style_gain"])
    return s, sabs


def demod_ref(s, wsq):
    """-> d [n, cout]"""
    return torch.rsqrt(s.square() @ wsq.T + EPS)


# ---------------------------------------------------------------------------------------------- backward
FLOAT4_CIN, FALLBACK_CIN = (4, 64, 512, 1024), (20, 48, 768, 2048)
# (n, cin, cout, s_chunks, d_chunks): every cin of both forms of the demodulation product, every cout, every chunk pair (the per-row sums
# change form at 16 chunks and take a second trip over the lanes above 64), n = 1 and 3; the largest wsq is 8 MB
BACKWARD_CASES = [
    (1, 4, 3, 1, 1), (3, 64, 100, 15, 17), (3, 512, 2048, 16, 15), (1, 1024, 2048, 15, 17), (3, 1024, 3, 70, 16), (1, 64, 2048, 70, 16),
    (3, 512, 100, 2, 70),
    (1, 20, 100, 2, 70), (3, 48, 3, 16, 15), (3, 768, 100, 70, 16), (1, 2048, 100, 2, 70), (3, 2048, 3, 1, 1), (3, 20, 2048, 15, 17),
]
DEMOD_OFF_CASE = (3, 64, 100, 15, 17)
DEMOD_OFF_WAYS = ("all", "wsq", "d", "dc_part")                       # which pointers of the job are null
WDIM64_CASE = (3, 64, 100, 16, 15)
MIXED_JOBS = ((64, 100, 15, 17), (48, 3, 16, 15), (768, 100, 70, 16))  # one launch, n = 3, next to a job without demodulation and an attention job


def bwd_job(n, cin, cout, s_chunks, d_chunks, wdim=WDIM, seed=None):
    """Seeded operands of one style-gradient job.  s and d are the float64 forward references ROUNDED TO FLOAT32: the kernel is handed
    them, and the float64 reference of the adjoint is evaluated on the same numbers, so no forward error enters the comparison."""
    torch.manual_seed(7000 + 1000 * n + 3 * cin + cout + 31 * s_chunks + d_chunks + wdim if seed is None else seed)
    roles = roles_for(n)
    wg = _scale_rows(f32r(torch.randn(n, wdim, dtype=F64)), roles)
    job = dict(cin=cin, cout=cout, aff_w=f32r(torch.randn(cin, wdim, dtype=F64)), wsq=make_wsq(cout, cin), s_chunks=s_chunks, d_chunks=d_chunks,
               aff_gain=float(f32r(torch.tensor(1.0 / math.sqrt(wdim)))), style_gain=1.25, wg=wg,
               ds_part=f32r(torch.randn(n, cin, s_chunks, dtype=F64)), dc_part=f32r(torch.randn(n, cout, d_chunks, dtype=F64)))
    s = wg @ job["aff_w"].T * job["aff_gain"] * job["style_gain"]
    job["s"] = f32r(s)
    job["d"] = f32r(demod_ref(s, job["wsq"]))
    return job


def style_bwd_ref(job, demod=True, s=None, d=None):
    """-> ds [n, cin], dwg [n, wdim]"""
    s = job["s"] if s is None else s
    d = job["d"] if d is None else d
    ds = job["ds_part"].sum(-1)
    if demod:
        ds = ds - s * ((job["dc_part"].sum(-1) * d.square()) @ job["wsq"])
    return ds, job["aff_gain"] * job["style_gain"] * (ds @ job["aff_w"])


# ---------------------------------------------------------------------------------------------- operator level
# (n, cin, cout, roles)
DEMOD_OP_CASES = [(2, 5, 4100, (NORMAL, ZERO)),                       # more rows than 1024 blocks x 4 waves: the stride loop
                  (3, 2048, 3, (NORMAL, SMALL, ZERO)), (1, 1, 1, (NORMAL,))]
DEMOD_BWD_OP_CASES = [(2, 257, 3, (NORMAL, SMALL)),                   # two blocks of 256 lanes, the second with one
                      (1, 20, 2048, (NORMAL,)), (3, 512, 100, (NORMAL, SMALL, ZERO))]


def demod_op_inputs(n, cin, cout, roles):
    torch.manual_seed(8000 + 100 * n + cin + cout)
    s = f32r(_scale_rows(torch.randn(n, cin, dtype=F64), roles))
    wsq = make_wsq(cout, cin)
    return dict(s=s, wsq=wsq, d=f32r(demod_ref(s, wsq)), dd=f32r(torch.randn(n, cout, dtype=F64)))


def demod_bwd_ref(dd, d, s, wsq):
    """-> ds_op [n, cin]"""
    return -s * ((dd * d.pow(3)) @ wsq)


# ---------------------------------------------------------------------------------------------- measures
def rows_rel(got, ref):
    """max over samples of (largest error of the sample's row) / (largest reference element of that row): the dot-product gate, per
    sample -- the SMALL sample's gradient is a thousand times a NORMAL one's and would otherwise set the scale for all of them.  A row
    whose reference is all zero must be reproduced exactly (-> inf otherwise)."""
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64).cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs().reshape(ref.shape[0], -1).amax(1)
    top = ref.abs().reshape(ref.shape[0], -1).amax(1)
    q = torch.where(err == 0, torch.zeros_like(err), err / top)       # (x / 0 = inf for x > 0)
    return float(q.max())


def scaled_err(got, ref, scale):
    """max |got - ref| / scale per element; an element whose scale is 0 must be exact."""
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64).cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / scale).max())


# ---------------------------------------------------------------------------------------------- the formulas in float32
def _sum32(terms):
    """Sequential float32 sum over the LAST axis, every partial sum rounded to float32 (torch's own reductions keep wider ones)."""
    acc = torch.zeros(terms.shape[:-1], dtype=torch.float32)
    for k in range(terms.shape[-1]):
        acc = acc + terms[..., k]
    return acc


def _dot32(a, b):
    """a [n, K] . b [K, m] -> [n, m], products and partial sums in float32, k ascending."""
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k in range(a.shape[1]):
        acc = acc + a[:, k:k + 1] * b[k][None]
    return acc


def styles_f32(ws, job):
    f = torch.float32
    acc = _dot32(ws[:, job["slot"]].to(f), job["aff_w"].to(f).T.contiguous())
    return (acc * job["aff_gain"] + job["aff_b"].to(f)[None]) * job["style_gain"]        # (the gains are float32 numbers)


def demod_f32(s, wsq):
    f = torch.float32
    s = s.to(f)
    return torch.rsqrt(_dot32(s * s, wsq.to(f).T.contiguous()) + torch.tensor(EPS, dtype=f))


def style_bwd_f32(job, demod=True):
    f = torch.float32
    s, d = job["s"].to(f), job["d"].to(f)
    ds = _sum32(job["ds_part"].to(f))
    if demod:
        ds = ds - s * _dot32(_sum32(job["dc_part"].to(f)) * d * d, job["wsq"].to(f))
    return ds, _dot32(ds, job["aff_w"].to(f)) * job["aff_gain"] * job["style_gain"]


def demod_bwd_f32(dd, d, s, wsq):
    f = torch.float32
    dd, d, s = dd.to(f), d.to(f), s.to(f)
    return -s * _dot32(dd * d * d * d, wsq.to(f))
