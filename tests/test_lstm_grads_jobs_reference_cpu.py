"""CPU part of the weight-gradient job tests (``tests/test_lstm_grads_jobs_gpu.py``): the job table
covers the dispatch space of the job launches, the float64 reference is checked a second way (autograd
of the products it stands for), and the discriminating power of the GPU bounds is asserted from the
reference alone: each mutant lies at least 5 bounds away on every job it applies to."""
import pytest
import torch

import test_lstm_grads_jobs_gpu as S

_JOBS = list(S.ALL_JOBS.values())
_IDS = [j.name for j in _JOBS]


def test_job_table_covers_the_dispatch_space():
    din_tiles = lambda j: (j.Dw + 16) // 16
    every = {(H, dt) for H in S.JOB_H for dt in (1, 2, 3, 4, 5)}
    assert {(j.H, din_tiles(j)) for j in S.SINGLE_JOBS} == every
    assert {(j.H, din_tiles(j)) for j in S.FLUSH_JOBS} == every
    assert any(j.seq for j in S.SINGLE_JOBS)
    assert len(S.BATCH_JOBS) == S.MULTI_MAX == 12 and len({j.name for j in S.BATCH_JOBS}) == 12
    assert {j.H for j in S.BATCH_JOBS} == set(S.JOB_H) and {din_tiles(j) for j in S.BATCH_JOBS} == {1, 2, 3, 4, 5}
    assert {j.seq for j in S.BATCH_JOBS} == {False, True} and {j.splits for j in S.BATCH_JOBS} == {0, 2, 4}
    assert {(HR, a.H // HR) for HR, a, _ in S.REC_CASES} == {(HR, k) for HR in S.REC_H for k in (1, 2)}
    assert all(a.H == b.H for _, a, b in S.REC_CASES)
    # the reduction's narrow form (one slot block per workgroup) up to H = 32, the wide form from H = 64
    wide = lambda j: (S.record_floats(j.H, j.Dw) + 15) // 16 > 1024
    assert all(wide(j) == (j.H >= 64) for j in _JOBS)
    assert all(S.ldx_of(j.Dw) % 4 == 0 and 0 <= S.ldx_of(j.Dw) - j.Dw < 4 for j in _JOBS)
    assert S.T * S.MP == 96 and set(S.BOUNDS) == set(S.FAMILIES)
    assert float(torch.tensor(S.PREFILL).to(torch.bfloat16)) == S.PREFILL


@pytest.mark.parametrize("job", _JOBS, ids=_IDS)
def test_job_inputs_are_bf16_exact_and_reference_is_autograd(job):
    d, ref = S.job_case(job)
    for n in ("x", "h", "dz"):
        assert torch.equal(S._bf(d[n]), d[n]), n
    # dW, dU, db as float64 autograd of sum(dz * (x W + h_{t-1} U + b)) over the job's row mapping
    lead = (S.MP, S.T) if job.seq else (S.T, S.MP)
    x, h, dz = (d[n].double().view(*lead, -1) for n in ("x", "h", "dz"))
    taxis = 1 if job.seq else 0
    hprev = torch.cat([torch.zeros_like(h.narrow(taxis, 0, 1)), h.narrow(taxis, 0, S.T - 1)], taxis)
    W = torch.zeros(job.Dw, 4 * job.H, dtype=torch.float64, requires_grad=True)
    U = torch.zeros(job.H, 4 * job.H, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(4 * job.H, dtype=torch.float64, requires_grad=True)
    gW, gU, gb = torch.autograd.grad((dz * (x @ W + hprev @ U + b)).sum(), [W, U, b])
    for q, g in (("dW", gW), ("dU", gU), ("db", gb)):
        assert (ref[q] - g).abs().max().item() <= 1e-12 * max(1.0, g.abs().max().item()), (job.name, q)


@pytest.mark.parametrize("job", _JOBS, ids=_IDS)
def test_every_mutant_is_five_bounds_away(job):
    d, ref = S.job_case(job)
    bound = max(S.BOUNDS.values())
    for mut, q in (("h_t", "dU"), ("no_bias", "db")):
        m = S.job_reference(job, d, mut)
        dist = S.rel_err(m[q], ref[q])
        assert dist / bound >= S.MUTANT_FACTOR, f"{job.name}: mutant {mut} moves {q} by {dist:.3e}"
        for other in {"dW", "dU", "db"} - {q}:
            assert torch.equal(m[other], ref[other])
        print(f"JOBMUT {job.name} {mut} {dist / bound:.1f}")
