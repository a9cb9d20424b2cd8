"""Weight-gradient job launches (``csrc/kernels/lstm_grads_jobs.hip``: ``lstm_grads_multi`` and
``lstm_tm_bwd_pipe``) called directly through ``hip_ops()`` over their (job hidden size, din tiles,
recurrence hidden size) dispatch space, against a float64 reference on the CPU.

A job is (dz, x, h, W, period, hshift, workspace): ``dW += x^T dz``, ``dU += h_{t-1}^T dz``,
``db += sum dz`` over flat rows, h_{t-1} of row r being row r - hshift where r % period >= hshift (else
0). Every job here has 96 rows = three 32-row tiles: time-major T = 3, Mp = 32 (period = T Mp,
hshift = Mp, bf16 dz), and one sequence-major job (M = 32, T = 3: period = T, hshift = 1, fp32 dz, which
the host rounds to bf16 before the launch). H in {16, 32, 64, 128} (the reduction's narrow form up to
32, its wide form from 64), Dw in {15, 16, 47, 48, 79} (1..5 din tiles incl. the bias row) with the x
row pitch padded to a multiple of 4 (x is a strided view; the pad channels hold 1.0 and must be
ignored). All inputs are drawn and then rounded to bf16, so the float64 reference is exact up to the
kernels' fp32 accumulation.

Routes: (a) ``lstm_grads_multi`` with one job, (b) with 12 jobs of mixed (H, din tiles, splits) and
their 12 reductions in the same call, (c) the flush form of ``lstm_tm_bwd_pipe`` (no recurrence): a
job launch, then a reduce launch, (d) ``lstm_tm_bwd_pipe`` with a recurrence of HR in {16, 32, 64}
carrying a job of HR or 2 HR and the reduction of an earlier job: the returned dz is bitwise the dz
of the same call without job and reduce, and ``lstm_dx(dz, W)`` is compared with ``lstm_tm_bwd``'s
frozen-path dx of the same state, (e) gradient buffers pre-filled with 0.5 (result = reference + 0.5),
(f) the refusals.

Metric and bounds: relative Frobenius error per tensor; one bound per family (:data:`BOUNDS`), 3 x the
family's worst error measured on an MI355X, rounded up to one significant digit (the project's rule,
``profiles/lstm_tm_kernel_tests.txt``); the per-case figures are in
``profiles/lstm_grads_jobs_tests.txt``. ``tests/test_lstm_grads_jobs_reference_cpu.py`` asserts from
the reference alone that the mutants ``h_t`` (h_t for h_{t-1} in dU) and ``no_bias`` (the bias row
dropped: db = 0) lie at least 5 bounds away on every job.
"""
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

T, MP = 3, 32                               # 96 rows: three 32-row tiles
JOB_H = (16, 32, 64, 128)
JOB_DW = (15, 16, 47, 48, 79)               # din tiles (Dw + 16) // 16 = 1 .. 5
REC_H = (16, 32, 64)
REC_DIN = 20
PREFILL = 0.5                               # bf16-exact
MULTI_MAX = 12                              # lstm_grads_jobs.hip MULTI_MAX
FAMILIES = ("multi", "flush", "rec")
# 3 x the worst error measured in the family on an MI355X, rounded up to one significant digit
# (profiles/lstm_grads_jobs_tests.txt)
BOUNDS = {"multi": 2e-7, "flush": 2e-7, "rec": 2e-7}
MUTANT_FACTOR = 5.0

Job = namedtuple("Job", "name H Dw seq splits seed")


def _j(H, Dw, seq=False, splits=0, seed=0):
    """splits = 0: the workspace of ``lstm_grads_job_ws`` (one split at 96 rows), else that many records."""
    return Job(f"h{H}_d{Dw}" + ("_seq" if seq else "") + (f"_s{splits}" if splits else "") + (f"_r{seed}" if seed else ""),
               H, Dw, seq, splits, seed)


SINGLE_JOBS = [_j(H, Dw) for H in JOB_H for Dw in JOB_DW] + [_j(32, 47, seq=True)]
# 12 jobs in one launch: every H, every din tile count, both row mappings, 1 / 2 / 4 (> tiles) splits
BATCH_JOBS = [_j(16, 15, splits=2), _j(128, 79), _j(32, 47, seq=True), _j(64, 16, splits=4), _j(16, 48),
              _j(32, 16, splits=2), _j(128, 15, splits=2), _j(64, 79, splits=2), _j(32, 79), _j(16, 47, splits=4),
              _j(64, 48), _j(128, 47, seq=True, splits=2)]
FLUSH_JOBS = [_j(H, Dw, splits=(2 if (H // 16 + Dw) % 2 else 0)) for H in JOB_H for Dw in JOB_DW]
PREFILL_JOBS = [_j(32, 47), _j(64, 16, splits=2), _j(128, 79)]
# (HR, riding job, earlier job whose reduction rides)
REC_CASES = [(HR, _j(k * HR, Dw, splits=sp, seed=1), _j(k * HR, Dw2, seed=2))
             for HR, k, Dw, Dw2, sp in ((16, 1, 15, 48, 0), (16, 2, 48, 16, 2), (32, 1, 79, 15, 0), (32, 2, 16, 47, 2),
                                        (64, 1, 47, 79, 2), (64, 2, 79, 16, 0))]
ALL_JOBS = {j.name: j for j in SINGLE_JOBS + BATCH_JOBS + FLUSH_JOBS + PREFILL_JOBS +
            [j for _, a, b in REC_CASES for j in (a, b)]}


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def ldx_of(Dw):
    return (Dw + 3) // 4 * 4


def record_floats(H, Dw):
    """Floats of one split record: [column blocks][din tiles + H / 16][1024]."""
    return ((Dw + 16) // 16 + H // 16) * 1024 * (4 * H // 64)


def job_inputs(j):
    """CPU float32 tensors of a job, bf16-exact, seeded by its shape: flat-row views x [rows, Dw],
    h [rows, H], dz [rows, 4H] plus (period, hshift)."""
    gen = torch.Generator().manual_seed(7300 + 977 * j.H + 13 * j.Dw + (5 if j.seq else 0) + 101 * j.seed)
    rows = T * MP
    d = dict(x=_bf(torch.randn(rows, j.Dw, generator=gen)), h=_bf(torch.randn(rows, j.H, generator=gen) * 0.5),
             dz=_bf(torch.randn(rows, 4 * j.H, generator=gen)), W=torch.randn(j.Dw, 4 * j.H, generator=gen) * 0.3)
    d["period"], d["hshift"] = (T, 1) if j.seq else (T * MP, MP)
    return d


def job_reference(j, d, mut=None):
    """float64 (dW, dU, db) of a job; ``mut``: 'h_t' (h_t for h_{t-1}) or 'no_bias' (the bias row dropped)."""
    x, h, dz = d["x"].double(), d["h"].double(), d["dz"].double()
    rows = x.shape[0]
    r = torch.arange(rows)
    hprev = torch.zeros_like(h)
    hprev[d["hshift"]:] = h[:rows - d["hshift"]]
    hprev[r % d["period"] < d["hshift"]] = 0
    if mut == "h_t":
        hprev = h
    db = dz.sum(0)
    if mut == "no_bias":
        db = torch.zeros_like(db)
    return dict(dW=x.t() @ dz, dU=hprev.t() @ dz, db=db)


_REFERENCES = {}


def job_case(j):
    """(inputs, reference) of a job, computed once per process and shared (never modified)."""
    if j.name not in _REFERENCES:
        d = job_inputs(j)
        _REFERENCES[j.name] = (d, job_reference(j, d))
    return _REFERENCES[j.name]


def rel_err(a, r):
    return (a - r).norm().item() / r.norm().item()


# ------------------------------------------------------------------ device side
def device_job(j, dev, prefill=0.0):
    """The job's device tensors: x as a [.., Dw] view of a [.., ldx] buffer whose pad channels hold 1.0."""
    from gnnqc.utils.native import hip_ops
    d, _ = job_case(j)
    lead = (MP, T) if j.seq else (T, MP)
    xb = torch.ones(*lead, ldx_of(j.Dw), device=dev)
    xb[..., :j.Dw] = d["x"].view(*lead, j.Dw).to(dev)
    x = xb[..., :j.Dw]
    dz = d["dz"].view(*lead, 4 * j.H).to(dev)
    if not j.seq:
        dz = dz.to(torch.bfloat16)
    h, W = d["h"].view(*lead, j.H).to(dev), d["W"].to(dev)
    ws = hip_ops().lstm_grads_job_ws(dz, x, W, j.H) if j.splits == 0 else \
        torch.empty(j.splits * record_floats(j.H, j.Dw), device=dev)
    assert ws.numel() % record_floats(j.H, j.Dw) == 0
    g = [torch.full((j.Dw, 4 * j.H), prefill, device=dev), torch.full((j.H, 4 * j.H), prefill, device=dev),
         torch.full((4 * j.H,), prefill, device=dev)]
    return dict(dz=dz, x=x, h=h, W=W, period=d["period"], hshift=d["hshift"], ws=ws, g=g)


def multi(jobs, reds):
    from gnnqc.utils.native import hip_ops
    hip_ops().lstm_grads_multi([k["dz"] for k in jobs], [k["x"] for k in jobs], [k["h"] for k in jobs],
                               [k["W"] for k in jobs], [k["period"] for k in jobs], [k["hshift"] for k in jobs],
                               [k["ws"] for k in jobs], [k["ws"] for k in reds], [k["W"] for k in reds],
                               [k["g"][0] for k in reds], [k["g"][1] for k in reds], [k["g"][2] for k in reds], [], [])


def pipe(rec=None, job=None, red=None, T_rec=0):
    """One ``lstm_tm_bwd_pipe`` launch: [recurrence (dh, g, c, W, U)] + [job] + [reduce]; returns dz."""
    from gnnqc.utils.native import hip_ops
    ref = rec[0] if rec is not None else (job or red)["ws"]
    e = ref.new_zeros(0)
    r = rec if rec is not None else (e, e, e, e, e)
    jb = (job["dz"], job["x"], job["h"], job["W"], job["period"], job["hshift"], job["ws"]) if job else \
        (e, e, e, e, 1, 1, e)
    rd = (red["ws"], red["W"], *red["g"]) if red else (e, e, e, e, e)
    return hip_ops().lstm_tm_bwd_pipe(*r, int(T_rec), *jb, *rd)


def check_job(family, route, j, k, prefill=0.0):
    """Every gradient of device job ``k`` within the family's bound of job ``j``'s reference."""
    _, ref = job_case(j)
    failures = []
    for q, a in zip(("dW", "dU", "db"), k["g"]):
        e = rel_err(a.double().cpu() - prefill, ref[q])
        print(f"JOBERR {family} {route} {j.name} {q} {e:.3e}")
        if not e <= BOUNDS[family]:
            failures.append(f"{j.name} {q}: {e:.3e} > {BOUNDS[family]:.0e}")
    return failures


def rec_state(HR, dev):
    """A saved-gates forward of one H = HR layer at (T, MP, REC_DIN) and a gradient of its output."""
    from gnnqc.utils.native import hip_ops
    gen = torch.Generator().manual_seed(8800 + HR)
    x = torch.randn(T, MP, REC_DIN, generator=gen).to(dev)
    W, U, b = ((torch.randn(REC_DIN, 4 * HR, generator=gen) * 0.3).to(dev),
               (torch.randn(HR, 4 * HR, generator=gen) * 0.3).to(dev), (torch.randn(4 * HR, generator=gen) * 0.1).to(dev))
    dh = torch.randn(T, MP, HR, generator=gen).to(dev)
    h, g, c = hip_ops().lstm_tm_fwd(x, W, U, b, True, True)
    return dict(x=x, W=W, U=U, b=b, dh=dh, h=h, g=g, c=c)


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("job", SINGLE_JOBS, ids=[j.name for j in SINGLE_JOBS])
def test_multi_single_job(cuda_device, job):
    """(a) one job and its reduction in one ``lstm_grads_multi`` call."""
    k = device_job(job, cuda_device)
    multi([k], [k])
    torch.cuda.synchronize()
    failures = check_job("multi", "a", job, k)
    assert not failures, "; ".join(failures)


def test_multi_twelve_mixed_jobs(cuda_device):
    """(b) 12 jobs of mixed (H, din tiles, row mapping, splits) in one launch, their reductions in the same
    call: each job's workgroups must run its own instance on its own data (start / key mapping)."""
    assert len(BATCH_JOBS) == MULTI_MAX
    ks = [device_job(j, cuda_device) for j in BATCH_JOBS]
    multi(ks, ks)
    torch.cuda.synchronize()
    failures = [f for j, k in zip(BATCH_JOBS, ks) for f in check_job("multi", "b", j, k)]
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("job", FLUSH_JOBS, ids=[j.name for j in FLUSH_JOBS])
def test_pipe_flush_job_then_reduce(cuda_device, job):
    """(c) ``lstm_tm_bwd_pipe`` without a recurrence: a job launch, then a reduce launch."""
    k = device_job(job, cuda_device)
    assert pipe(job=k).numel() == 0
    assert pipe(red=k).numel() == 0
    torch.cuda.synchronize()
    failures = check_job("flush", "c", job, k)
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("case", REC_CASES, ids=[f"hr{c[0]}_{c[1].name}" for c in REC_CASES])
def test_pipe_recurrence_with_riding_job(cuda_device, case):
    """(d) a recurrence carrying a job of HR or 2 HR and the reduction of an earlier job."""
    from gnnqc.utils.native import hip_ops
    ops = hip_ops()
    HR, job, earlier = case
    s = rec_state(HR, cuda_device)
    rec = (s["dh"], s["g"], s["c"], s["W"], s["U"])
    k0, k1 = device_job(earlier, cuda_device), device_job(job, cuda_device)
    pipe(job=k0)
    dz_alone = pipe(rec=rec, T_rec=T)
    dz = pipe(rec=rec, job=k1, red=k0, T_rec=T)
    pipe(red=k1)
    e = s["x"].new_zeros(0)
    dx_frozen = ops.lstm_tm_bwd(s["dh"], s["g"], s["c"], s["x"], s["h"], s["W"], s["U"], s["b"], e, e, e, True, None, 0)
    dx = ops.lstm_dx(dz, s["W"], s["x"])
    torch.cuda.synchronize()
    assert tuple(dz.shape) == (T + 1, MP, 4 * HR) and dz.dtype == torch.bfloat16
    assert torch.equal(dz[:T].view(torch.int16), dz_alone[:T].view(torch.int16)), "dz changed by the riding work"
    failures = check_job("rec", "d", earlier, k0) + check_job("rec", "d", job, k1)
    err = rel_err(dx.double().cpu(), dx_frozen.double().cpu())
    print(f"JOBERR rec d hr{HR}_{job.name} dx {err:.3e}")
    if not err <= BOUNDS["rec"]:
        failures.append(f"dx: {err:.3e} > {BOUNDS['rec']:.0e}")
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("job", PREFILL_JOBS, ids=[j.name for j in PREFILL_JOBS])
def test_gradients_are_accumulated(cuda_device, job):
    """(e) gradient buffers pre-filled with a bf16-exact constant: reference + constant, by both routes."""
    k = device_job(job, cuda_device, PREFILL)
    multi([k], [k])
    kp = device_job(job, cuda_device, PREFILL)
    pipe(job=kp)
    pipe(red=kp)
    torch.cuda.synchronize()
    failures = check_job("multi", "e", job, k, PREFILL) + check_job("flush", "e", job, kp, PREFILL)
    assert not failures, "; ".join(failures)


def test_job_launches_refuse_unsupported_arguments(cuda_device):
    """(f) argument combinations the host refuses (a check before any launch)."""
    from gnnqc.utils.native import hip_ops
    ops, dev = hip_ops(), cuda_device
    s = rec_state(16, dev)
    rec = (s["dh"], s["g"], s["c"], s["W"], s["U"])
    with pytest.raises(RuntimeError, match="job hidden size must be"):       # neither HR nor 2 HR
        pipe(rec=rec, job=device_job(_j(64, 16), dev), T_rec=T)
    k = device_job(_j(32, 47), dev)
    bad = dict(k, ws=torch.empty(k["ws"].numel() + 1, device=dev))
    with pytest.raises(RuntimeError, match="job workspace size"):
        pipe(job=bad)
    with pytest.raises(RuntimeError, match="reduce workspace size"):
        pipe(red=bad)
    with pytest.raises(RuntimeError, match="workspace size"):
        multi([bad], [])
    with pytest.raises(RuntimeError, match="job lists"):                     # 13 jobs
        multi([k] * (MULTI_MAX + 1), [])
    e = torch.zeros(0, device=dev)
    with pytest.raises(RuntimeError, match="GCN job rides"):                 # a GCN list without a gradient job
        ops.lstm_grads_multi([], [], [], [], [], [], [], [], [], [], [], [], [e] * 21, [0, 0, 0, 0])
    torch.cuda.synchronize()
