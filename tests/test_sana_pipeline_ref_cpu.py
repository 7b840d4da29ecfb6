"""The references of tests/sana_pipeline_ref.py checked against facts that do not come from them: the schedule's end points and shape, the exact
solution of the solver's own model problem (a constant x0 prediction), the orders of the two updates on a scalar ODE, and the distance of the fp32
op sequence from the float64 update. No GPU, no library."""
import math

import numpy as np
import pytest
import torch

from tests import sana_pipeline_ref as R

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("n", (1, 2, 20))
def test_schedule_facts(n):
    ts, sig = R.schedule(n)
    assert len(ts) == n and len(sig) == n + 1 and ts.dtype == np.int64
    assert sig[0] == pytest.approx(3 * 0.999 / (1 + 2 * 0.999), rel=1e-15) and sig[-1] == 0.0
    assert np.all(np.diff(sig) < 0)                                              # strictly decreasing, the appended 0 included
    assert ts[0] == 999 and np.array_equal(ts, np.floor(sig[:-1] * 1000).astype(np.int64))       # truncated, not rounded: 999.67 -> 999
    assert np.all(sig[:-1] * 1000 - ts < 1) and np.any(sig[:-1] * 1000 - ts > 0.5)
    # the unshifted sequence is linear in the step: undo the shift
    s = sig[:-1] / (3 - 2 * sig[:-1])
    assert np.allclose(s, np.linspace(0.999, 0, n + 1)[:-1], rtol=0, atol=1e-15)
    assert [R.step_order(i, n) for i in range(n)] == ([1] if n == 1 else [1] + [2] * (n - 2) + [1])


@pytest.mark.parametrize("n", (2, 20))
@pytest.mark.parametrize("solver_order", (1, 2))
def test_a_constant_x0_prediction_is_integrated_exactly(n, solver_order):
    """x0(x, t) = c: DPM-Solver++ of either order gives a x + alpha_t (1 - exp(-h)) c at every step, and the last step (sigma_t = 0) returns c"""
    _, sig = R.schedule(n)
    g = torch.Generator().manual_seed(n)
    c, x = torch.randn(64, generator=g, dtype=F64), torch.randn(64, generator=g, dtype=F64)
    m1 = None
    for i in range(n):
        order, s0, a, b, rinv, h = R.coefficients(sig, i, solver_order)
        flow = (x - c) / s0                                                      # the flow prediction whose x0 is c
        want = a * x + (1 - sig[i + 1]) * (1 - math.exp(-h)) * c
        x, m1 = R.dpm_step_f64(flow, None, 1.0, x, m1, order, s0, a, b, rinv)
        assert torch.allclose(x, want, rtol=1e-13, atol=1e-13) and torch.allclose(m1, c, rtol=1e-13, atol=1e-13), i
    assert (order, a, b) == (1, 0.0, -1.0) and math.isinf(h) and torch.allclose(x, c, rtol=1e-13, atol=1e-13)


def _toy_error(n, solver_order):
    """flow model v(x, s) = x cos(s): dx/ds = v has the solution x(s) = x(s_0) exp(sin s - sin s_0). n steps over the fixed interval sigma = 0.9 .. 0.1, away
    from both ends of the schedule, where lambda is unbounded and a step's h does not shrink with n; the appended 0 is never stepped to"""
    sig = np.concatenate([np.linspace(0.9, 0.1, n + 1), [0.0]])
    x, m1 = torch.tensor([1.0], dtype=F64), None
    for i in range(n):
        order, s0, a, b, rinv, _ = R.coefficients(sig, i, solver_order)
        assert order == (1 if i == 0 else solver_order)
        x, m1 = R.dpm_step_f64(x * math.cos(s0), None, 1.0, x, m1, order, s0, a, b, rinv)
    return abs(float(x) - math.exp(math.sin(0.1) - math.sin(0.9)))


def test_second_order_converges_faster_on_a_smooth_ode():
    e1 = [_toy_error(n, 1) for n in (20, 40)]
    e2 = [_toy_error(n, 2) for n in (20, 40)]
    print(f"toy ODE: first order {e1[0]:.3e} -> {e1[1]:.3e} (x {e1[0] / e1[1]:.2f}), second order {e2[0]:.3e} -> {e2[1]:.3e} (x {e2[0] / e2[1]:.2f})")
    assert e2[0] / e2[1] > e1[0] / e1[1] and e2[1] < e1[1]


@pytest.mark.parametrize("guided", (False, True))
@pytest.mark.parametrize("n", (2, 20))
def test_fp32_op_sequence_stays_within_a_few_ulps_of_float64(n, guided):
    """The distance is counted in fp32 ulps of the update's SCALE, the sum of the magnitudes of its terms (a result that cancels has no ulp of its own to
    count in). At most 12 roundings lie between the inputs and the sample (3 guidance, 2 conversion, 3 first order, 4 second order), each at most half
    an ulp of a value the scale bounds, and the scale may sit at the top of its binade: 12 x 0.5 x 2 = 12 ulps. Measured over these cases (sample and x0):
    1.79 and 2.26 ulps without guidance (n = 2, 20), 2.57 and 3.06 with."""
    _, sig = R.schedule(n)
    s32 = torch.from_numpy(sig.astype(np.float32))
    N, gs = 1 << 14, 4.5
    worst = 0.0
    for i in range(n):
        g = torch.Generator().manual_seed(100 * n + i)
        u, x, m1 = (torch.randn(N, generator=g) for _ in range(3))
        t = torch.randn(N, generator=g) if guided else None
        order, s0, a, b, rinv = R.coefficients_f32(s32, i)
        o, x0, mi = R.dpm_step_f32_ops(u, t, gs, x, m1, order, s0, a, b, rinv)
        o64, x064 = R.dpm_step_f64(u, t, gs, x, m1, order, s0, a, b, rinv)
        assert o.dtype == F32 and x0.dtype == F32 and torch.equal(mi, o)
        pm = u.double().abs() + (gs * (t.double().abs() + u.double().abs()) if guided else 0)
        x0m = x.double().abs() + s0 * pm
        scale = abs(a) * x.double().abs() + abs(b) * x0m + (abs(0.5 * b * rinv) * (x0m + m1.double().abs()) if order == 2 else 0)
        ulp = lambda s: 2.0 ** (torch.floor(torch.log2(s)) - 23)
        worst = max(worst, float(((o.double() - o64).abs() / ulp(scale)).max()), float(((x0.double() - x064).abs() / ulp(x0m)).max()))
    print(f"fp32 op sequence vs float64, n = {n}, guided = {guided}: {worst:.2f} ulps of the scale (bound 12)")
    assert worst <= 12


def test_fp32_coefficients_follow_the_float64_ones():
    for n in (1, 2, 20):
        _, sig = R.schedule(n)
        s32 = torch.from_numpy(sig.astype(np.float32))
        for i in range(n):
            o32, o64 = R.coefficients_f32(s32, i), R.coefficients(sig, i)[:5]
            assert o32[0] == o64[0] and np.allclose(o32[1:], o64[1:], rtol=2e-5, atol=0), (n, i, o32, o64)
            assert all(float(np.float32(v)) == v for v in o32[1:])                  # fp32 values
        assert o32[2:4] == (0.0, -1.0)


def test_special_values_hold_what_they_promise():
    for dt in (torch.bfloat16, F32):
        v = R.special_values(2040, dt, 3).float()
        assert (v == 0).sum() >= 2 and torch.signbit(v[v == 0]).any() and ((v != 0) & (v.abs() < 2.0 ** -126)).any() and (v.abs() > 3e38).any()
        assert torch.isfinite(v).all()
