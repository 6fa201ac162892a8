"""The Euler / classifier-free-guidance loop of `oracle.flow.cfm_solve` restated with a guidance rate PER STEP and a choice of time
schedule (a plain module, not a conftest).  Only the loop is restated: every estimator evaluation is `oracle.flow.estimator`.

With a constant schedule `[r] * n` and the cosine scheduler this is `oracle.flow.cfm_solve(..., cfg_rate=r)` bit for bit -- the same
tensors through the same operations in the same order, a step of rate 0 included (it evaluates the unconditional rows as the
oracle does and weights them by 0) -- which tests/test_guidance_host.py asserts."""
import torch

from oracle import flow as oflow


def t_span(n_timesteps, t_scheduler="cosine"):
    """linspace(0, 1, n + 1), through 1 - cos(t pi / 2) for the cosine scheduler"""
    if t_scheduler == "cosine":
        return oflow.t_span(n_timesteps)
    assert t_scheduler == "linear", t_scheduler
    return torch.linspace(0, 1, n_timesteps + 1)


def cfm_solve(sd, noise, mu, mask, spks, cond, n_timesteps, temperature=1.0, rates=None, t_scheduler="cosine",
              pre="decoder.estimator."):
    """rates: n_timesteps guidance rates, step k of the loop uses rates[k] (None: 0.7 in every step)"""
    rates = [0.7] * n_timesteps if rates is None else [float(r) for r in rates]
    assert len(rates) == n_timesteps, (len(rates), n_timesteps)
    B, _, T = mu.shape
    x = noise[:, :, :T].expand(B, -1, -1) * temperature
    ts = t_span(n_timesteps, t_scheduler)
    t, dt = ts[0], ts[1] - ts[0]
    zeros = torch.zeros_like(mu)
    for step in range(1, n_timesteps + 1):
        r = rates[step - 1]
        d = oflow.estimator(sd, torch.cat([x, x], 0), torch.cat([mask, mask], 0), torch.cat([mu, zeros], 0), t.expand(2 * B),
                            torch.cat([spks, torch.zeros_like(spks)], 0), torch.cat([cond, zeros], 0), pre=pre)
        d = (1.0 + r) * d[:B] - r * d[B:]
        x = x + dt * d
        t = t + dt
        if step < n_timesteps:
            dt = ts[step + 1] - t
    return x.float()
