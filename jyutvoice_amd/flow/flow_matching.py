"""Configuration holder mirroring `jyutvoice.flow.flow_matching.CausalConditionalCFM` (flow_matching.py:343-401).

Unlike the reference constructor this one does not reseed the global torch / numpy / python RNGs
(flow_matching.py:353): the fixed noise tensor is drawn from a private seed-0 generator (synth.rand_noise).

The solver's two plain settings, `inference_cfg_rate` and `t_scheduler` (configs/base.yaml), are read from the configuration as
the reference's solver reads them (flow_matching.py:215-265, 387-389): the rate through the library's guidance mode
(jv_flow_set_guidance), the schedule through the t_span handed to the solve.  The helpers below are pure host functions."""
import math

import torch

from .. import spec

T_SCHEDULERS = ("cosine", "linear")


def _get(params, name):
    return params[name] if isinstance(params, dict) else getattr(params, name)


def check_scheduler(who: str, t_scheduler) -> str:
    if t_scheduler not in T_SCHEDULERS:
        raise ValueError(f"{who}: t_scheduler must be one of {list(T_SCHEDULERS)}, got {t_scheduler!r}")
    return t_scheduler


SOLVERS = ("euler", "midpoint", "heun")      # jv_flow_set_solver
EVALS = {"euler": 1, "midpoint": 2, "heun": 2}      # estimator evaluations per step


def check_solver(who: str, solver) -> str:
    if not isinstance(solver, str) or solver not in SOLVERS:
        raise ValueError(f"{who}: solver must be one of {list(SOLVERS)}, got {solver!r}")
    return solver


def check_rate(who: str, rate, name: str = "cfg_rate") -> float:
    """a guidance rate: finite and >= 0 (0: no guidance, the step needs no unconditional evaluation)"""
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not math.isfinite(rate) or rate < 0:
        raise ValueError(f"{who}: {name} must be a finite number >= 0, got {rate!r}")
    return float(rate)


def time_span(n_timesteps: int, t_scheduler: str = "cosine") -> torch.Tensor:
    """t_span of flow_matching.py:387-389: linspace(0, 1, n + 1), through 1 - cos(t pi / 2) for the cosine scheduler"""
    t = torch.linspace(0, 1, n_timesteps + 1)
    if check_scheduler("time_span()", t_scheduler) == "cosine":
        t = 1 - torch.cos(t * 0.5 * torch.pi)
    return t


def resolve_guidance(who: str, n_timesteps: int, configured: float, cfg_rate=None, cfg_schedule=None):
    """What a call hands Engine.set_guidance: None where the library's default (0.7 in every step) is what is asked for, else a
    list of one rate or of n_timesteps rates.  cfg_schedule (one rate per Euler step) wins over cfg_rate; cfg_rate = None means
    `configured`, the decoder's inference_cfg_rate."""
    if cfg_schedule is not None:
        rates = [check_rate(who, r, "cfg_schedule entry") for r in
                 (cfg_schedule.tolist() if isinstance(cfg_schedule, torch.Tensor) else list(cfg_schedule))]
        if len(rates) != n_timesteps:
            raise ValueError(f"{who}: cfg_schedule holds {len(rates)} rates, n_timesteps = {n_timesteps}: one per Euler step")
        return rates
    rate = check_rate(who, configured if cfg_rate is None else cfg_rate)
    return None if abs(rate - spec.CFG_RATE) <= 1e-12 else [rate]


def decoder_settings(decoder):
    """(inference_cfg_rate, t_scheduler, solver) of a decoder object; the reference's defaults where it carries none (its solver is
    solve_euler: "euler")"""
    return (float(getattr(decoder, "inference_cfg_rate", spec.CFG_RATE)), getattr(decoder, "t_scheduler", "cosine") or "cosine",
            getattr(decoder, "solver", "euler") or "euler")


def resolve_solver(who: str, configured: str, solver=None) -> str:
    """the solver of a call: `solver`, or the decoder's setting where it is None; a bad name raises ValueError naming the choices"""
    return check_solver(who, configured if solver is None else solver)


class CausalConditionalCFM:
    def __init__(self, in_channels, cfm_params, n_spks=1, spk_emb_dim=64, estimator=None):
        self.t_scheduler = _get(cfm_params, "t_scheduler")
        self.inference_cfg_rate = _get(cfm_params, "inference_cfg_rate")
        if spk_emb_dim != spec.N_FEATS:
            raise NotImplementedError("libjyutvoice_hip is built for spk_emb_dim=80 (configs/base.yaml:76-87)")
        if self.t_scheduler not in T_SCHEDULERS:
            raise NotImplementedError(f"libjyutvoice_hip knows t_scheduler 'cosine' and 'linear' (flow_matching.py:387-389), got "
                                      f"{self.t_scheduler!r}")
        self.inference_cfg_rate = check_rate("CausalConditionalCFM", self.inference_cfg_rate, "inference_cfg_rate")
        try:      # (an extension: the reference's only solver is solve_euler)
            self.solver = check_solver("CausalConditionalCFM", _get(cfm_params, "solver"))
        except (KeyError, AttributeError):
            self.solver = "euler"
        try:      # used by JyutVoiceTTS.forward only (flow_matching.py:330-334); base.yaml: 0.2
            self.training_cfg_rate = float(_get(cfm_params, "training_cfg_rate"))
        except (KeyError, AttributeError):
            self.training_cfg_rate = 0.2
        self.estimator = estimator
        self.device = torch.device("cuda:0")      # JyutVoiceTTS sets it to its own device

    @torch.inference_mode()
    def forward(self, mu, mask, n_timesteps, temperature=1.0, spks=None, cond=None, streaming=False, cfg_rate=None,
                cfg_schedule=None, solver=None):
        """flow_matching.py:356-401 -> (mel [B,80,T], None): fixed noise prefix * temperature, this decoder's t_scheduler, the
        Euler/CFG loop (solve_euler, :215-265) at this decoder's inference_cfg_rate -- all of it inside jv_cfm_solve.
        streaming=True: the estimator's chunk-causal attention (decoder.py:951-954) with this decoder's static_chunk_size, so
        frames of finished chunks do not change when more of the utterance arrives.  B > 1 is the batched extension (mask rows
        = per-utterance lengths).  cfg_rate / cfg_schedule (extensions): another rate for this call / one rate per step.
        solver (extension): "euler" / "midpoint" / "heun" for this call (None: this decoder's `solver`)."""
        from ..runtime import get_runtime
        B, _, T = mu.shape
        rates = resolve_guidance("CausalConditionalCFM.forward()", n_timesteps, self.inference_cfg_rate, cfg_rate, cfg_schedule)
        solver = resolve_solver("CausalConditionalCFM.forward()", self.solver, solver)
        eng = get_runtime(self.device).ensure(B, T, 1)
        chunk = getattr(self.estimator, "static_chunk_size", spec.EST_STATIC_CHUNK) if streaming else 0
        try:
            eng.set_streaming(chunk)
            if rates is not None:
                eng.set_guidance(rates)
            lens = None if mask is None else mask.reshape(B, -1).ne(0).sum(dim=1)
            if cond is None:
                cond = torch.zeros_like(mu)
            with eng.solver(solver):
                mel = eng.cfm_solve(mu, lens, spks, cond, n_timesteps, temperature, t_span=time_span(n_timesteps, self.t_scheduler))
        finally:
            eng.set_streaming(0)
            if rates is not None:
                eng.set_guidance(None)
        return mel, None

    __call__ = forward
