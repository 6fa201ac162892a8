"""`guidance_ref.cfm_solve`'s loop restated with a choice of integrator (a plain module, not a conftest).  Only the loop is
restated: every estimator evaluation is `oracle.flow.estimator`, and the state dict, the noise and the inputs may be of any float
dtype (the schedule stays on fp32 tensors, as the oracle keeps it).

With g(x, t) = (1 + r_k) d_cond - r_k d_uncond of step k and (t, dt) the running recurrence of `guidance_ref.cfm_solve`:

    euler      x <- x + dt g(x, t)                                            -- `guidance_ref.cfm_solve` bit for bit
    midpoint   xs = x + (0.5 dt) g(x, t);   x <- x + dt g(xs, t + 0.5 dt)
    heun       k1 = g(x, t);  xs = x + dt k1;   x <- x + (0.5 dt) (k1 + g(xs, t + dt))

which is the definition jv_flow_set_solver states (include/jyutvoice_hip.h).  tests/test_solver_host.py asserts the Euler identity."""
import torch

from guidance_ref import t_span
from oracle import flow as oflow

SOLVERS = ("euler", "midpoint", "heun")


def cfm_solve(sd, noise, mu, mask, spks, cond, n_timesteps, temperature=1.0, rates=None, t_scheduler="cosine", solver="euler",
              pre="decoder.estimator.", times=None):
    """rates: n_timesteps guidance rates, both evaluations of step k use rates[k] (None: 0.7 in every step).  times (optional
    list): receives the t of every estimator evaluation, as fp32 floats"""
    assert solver in SOLVERS, solver
    rates = [0.7] * n_timesteps if rates is None else [float(r) for r in rates]
    assert len(rates) == n_timesteps, (len(rates), n_timesteps)
    B, _, T = mu.shape
    x = noise[:, :, :T].expand(B, -1, -1) * temperature
    ts = t_span(n_timesteps, t_scheduler)
    t, dt = ts[0], ts[1] - ts[0]
    zeros = torch.zeros_like(mu)

    def g(x, t, r):
        if times is not None:
            times.append(float(t))
        d = oflow.estimator(sd, torch.cat([x, x], 0), torch.cat([mask, mask], 0), torch.cat([mu, zeros], 0), t.expand(2 * B),
                            torch.cat([spks, torch.zeros_like(spks)], 0), torch.cat([cond, zeros], 0), pre=pre)
        return (1.0 + r) * d[:B] - r * d[B:]

    for step in range(1, n_timesteps + 1):
        r = rates[step - 1]
        if solver == "euler":
            x = x + dt * g(x, t, r)
        elif solver == "midpoint":
            half = 0.5 * dt
            xs = x + half * g(x, t, r)
            x = x + dt * g(xs, t + half, r)
        else:
            k1 = g(x, t, r)
            xs = x + dt * k1
            x = x + (0.5 * dt) * (k1 + g(xs, t + dt, r))
        t = t + dt
        if step < n_timesteps:
            dt = ts[step + 1] - t
    return x if x.dtype == torch.float64 else x.float()
