"""Host-side mirror of Exmc.SMC (lib/exmc/smc.ex) over libexmc_hip.so.

    sample(ir, opts)               -> (trace, info)            smc.ex:19-44
    sample(ir, opts, num_runs=n)   -> ([trace], [info])        run r: seed + 7919 r

`trace` is {name: [num_particles, ...]} in constrained space (sampler._build_trace, as build_trace
:249-260 constrains the particles), `info` is the reference's {num_stages, betas, ess_history,
acceptance_rates} plus status: 0 when the run finished at beta = 1.0, 1 when max_stages ended it. One
particle sits on one lane group (include/exmc_hip_smc.h); the stage loop is on the host. For a built
model kind it is exmc_hip_smc_host's; for a generated model it runs here: the plug-in's init and
mutate and libexmc_hip.so's model-free reweight on the same device arrays, the split the pointwise
and fit-PSIS routes use. There is no CPU fallback. An IR without free variables (smc.ex:23-24) does
not reach this module: the generator refuses it.

    sample_bridged(ir, opts, base=None)  -> (trace, info)      DESIGN.md "Bridged SMC"

is the second mode (include/exmc_hip_smc_bridge.h): the temper runs along the geometric bridge from a
normalised diagonal normal, the base, to the model's density, the start is divided out of the weights,
every stage resamples, and info carries log_evidence, an estimate of log p(y), and log_evidence_steps.
The base is the start of `sample` (N(0, 0.25 I)) or a fit: (mu, sigma), or a dict with mu and sigma or
log_sigma -- an ADVI info, a Pathfinder result -- in the unconstrained kernel order.
pooled_log_evidence(infos) pools the estimates of a batch of runs."""
import ctypes as C
import math

import numpy as np

from . import _lib

# smc.ex:12-17
DEFAULT_OPTS = dict(num_particles=500, threshold_ratio=0.5, num_mh_steps=5, seed=0)


def _validate(opts, num_runs):
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    for key in ("num_particles", "num_mh_steps"):
        if int(o[key]) < 1:
            raise ValueError("%s must be >= 1" % key)
    if not math.isfinite(float(o["threshold_ratio"])):
        raise ValueError("threshold_ratio must be finite")
    if int(o.get("max_stages", _lib.SMC_DEFAULT_MAX_STAGES)) < 1:
        raise ValueError("max_stages must be >= 1")
    if int(num_runs) < 1:
        raise ValueError("num_runs must be >= 1")
    if int(o.get("run_lo", 0)) < 0:
        raise ValueError("run_lo must be >= 0")
    return o


def _c_opts(o):
    return _lib.SmcOpts(int(o["num_particles"]), float(o["threshold_ratio"]), int(o["num_mh_steps"]), int(o["seed"]),
                        int(o.get("max_stages", _lib.SMC_DEFAULT_MAX_STAGES)), int(o.get("lanes_per_chain") or 0))


def _is_generated(compiled):
    return getattr(compiled.spec, "lib_path", None) is not None


def _base(base, d):
    """(mu, sigma) as float64 [d], or (None, None): the default base. Checked here as the library checks it."""
    if base is None:
        return None, None
    if isinstance(base, dict):
        mu = base["mu"]
        sigma = base["sigma"] if base.get("sigma") is not None else np.exp(np.asarray(base["log_sigma"], dtype=np.float64))
    else:
        mu, sigma = base
    mu = np.ascontiguousarray(np.asarray(mu, dtype=np.float64).reshape(-1))
    sigma = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).reshape(-1))
    if mu.shape != (d,) or sigma.shape != (d,):
        raise ValueError("base: mu and sigma need %d entries, one fit" % d)
    if not (np.all(np.isfinite(mu)) and np.all(np.isfinite(sigma)) and np.all(sigma > 0.0)):
        raise ValueError("base: mu and sigma must be finite, sigma > 0")
    return mu, sigma


def sample_raw(compiled, opts=None, num_runs=1):
    """The arrays of exmc_hip_smc_host: particles [R][N][d] (unconstrained, kernel order), logp [R][N],
    betas, ess_history and acceptance_rates [R][max_stages] (NaN at and after num_stages), num_stages and
    status [R]. opts["run_lo"] offsets the seeds. kernel_ms is the sum over the call's kernels; for a
    generated model mutate_ms is the mutation's share."""
    o = _validate(opts, num_runs)
    if _is_generated(compiled):
        return _run_generated(compiled, o, int(num_runs))
    R, N, d = int(num_runs), int(o["num_particles"]), compiled.d
    S = int(o.get("max_stages", _lib.SMC_DEFAULT_MAX_STAGES))
    out = dict(particles=np.zeros((R, N, d)), logp=np.zeros((R, N)), betas=np.zeros((R, S)),
               ess_history=np.zeros((R, S)), acceptance_rates=np.zeros((R, S)), num_stages=np.zeros(R, np.int32),
               status=np.zeros(R, np.int32))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    compiled.check(compiled.L.exmc_hip_smc_host(
        compiled.h, _c_opts(o), R, int(o.get("run_lo", 0)),
        *[out[k].ctypes.data_as(dp) for k in ("particles", "logp", "betas", "ess_history", "acceptance_rates")],
        *[out[k].ctypes.data_as(ip) for k in ("num_stages", "status")]))
    out["kernel_ms"] = compiled.last_kernel_ms
    return out


def sample_bridged_raw(compiled, opts=None, num_runs=1, base=None):
    """The arrays of exmc_hip_smc_bridge_host: those of sample_raw, logb [R][N], log_evidence [R] and
    log_evidence_steps [R][max_stages] (NaN at and after num_stages)."""
    o = _validate(opts, num_runs)
    mu, sigma = _base(base, compiled.d)
    if _is_generated(compiled):
        return _run_generated(compiled, o, int(num_runs), bridged=True, mu=mu, sigma=sigma)
    R, N, d = int(num_runs), int(o["num_particles"]), compiled.d
    S = int(o.get("max_stages", _lib.SMC_DEFAULT_MAX_STAGES))
    out = dict(particles=np.zeros((R, N, d)), logp=np.zeros((R, N)), logb=np.zeros((R, N)), betas=np.zeros((R, S)),
               ess_history=np.zeros((R, S)), acceptance_rates=np.zeros((R, S)), num_stages=np.zeros(R, np.int32),
               status=np.zeros(R, np.int32), log_evidence=np.zeros(R), log_evidence_steps=np.zeros((R, S)))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    compiled.check(compiled.L.exmc_hip_smc_bridge_host(
        compiled.h, _c_opts(o), R, int(o.get("run_lo", 0)),
        mu.ctypes.data_as(dp) if mu is not None else dp(), sigma.ctypes.data_as(dp) if sigma is not None else dp(),
        *[out[k].ctypes.data_as(dp) for k in ("particles", "logp", "logb", "betas", "ess_history", "acceptance_rates")],
        *[out[k].ctypes.data_as(ip) for k in ("num_stages", "status")],
        *[out[k].ctypes.data_as(dp) for k in ("log_evidence", "log_evidence_steps")]))
    out["kernel_ms"] = compiled.last_kernel_ms
    return out


def _run_generated(compiled, o, R, bridged=False, mu=None, sigma=None):
    """init and mutate of the plug-in, reweight of libexmc_hip.so, on the same device arrays; bridged: their
    forms of include/exmc_hip_smc_bridge.h"""
    import torch
    from .diagnostics import _ordered_after_torch
    N, d = int(o["num_particles"]), compiled.d
    S = int(o.get("max_stages", _lib.SMC_DEFAULT_MAX_STAGES))
    Cn = R * N
    dev = torch.device("cuda", compiled.device)
    f8 = dict(dtype=torch.float64, device=dev)
    i4 = dict(dtype=torch.int32, device=dev)
    q, lp = torch.zeros((d, Cn), **f8), torch.zeros(Cn, **f8)
    words = torch.zeros((2, Cn), dtype=torch.int64, device=dev)
    t = dict(beta=torch.zeros(R, **f8), run_rng=torch.zeros((2, R), dtype=torch.int64, device=dev),
             active=torch.zeros(R, **i4), scale=torch.zeros((d, R), **f8), accept=torch.zeros(Cn, **i4),
             betas=torch.zeros((S, R), **f8), ess_history=torch.zeros((S, R), **f8),
             acceptance_rates=torch.zeros((S, R), **f8), num_stages=torch.zeros(R, **i4), status=torch.zeros(R, **i4),
             active_count=torch.zeros(1, **i4))
    st = _lib.SmcState(*[t[k].data_ptr() for k, _ in _lib.SmcState._fields_])
    co = _c_opts(o)
    main = _lib.load()
    L, h, lo = compiled.L, compiled.h, int(o.get("run_lo", 0))
    if bridged:
        lb, le, les = torch.zeros(Cn, **f8), torch.zeros(R, **f8), torch.zeros((S, R), **f8)
        mu_t = torch.from_numpy(mu).to(dev) if mu is not None else None
        sg_t = torch.from_numpy(sigma).to(dev) if sigma is not None else None
        mu_p, sg_p = (mu_t.data_ptr() if mu_t is not None else None), (sg_t.data_ptr() if sg_t is not None else None)

        def init():
            return L.exmc_hip_smc_bridge_init(h, co, R, lo, mu_p, sg_p, q.data_ptr(), lp.data_ptr(), lb.data_ptr(),
                                              words.data_ptr(), st, le.data_ptr(), les.data_ptr())

        def reweight(stage):
            return main.exmc_hip_smc_bridge_reweight(compiled.device, co, R, d, stage, q.data_ptr(), lp.data_ptr(),
                                                     lb.data_ptr(), st, le.data_ptr(), les.data_ptr())

        def mutate():
            return L.exmc_hip_smc_bridge_mutate(h, co, R, mu_p, sg_p, q.data_ptr(), lp.data_ptr(), lb.data_ptr(),
                                                words.data_ptr(), st)
    else:
        def init():
            return L.exmc_hip_smc_init(h, co, R, lo, q.data_ptr(), lp.data_ptr(), words.data_ptr(), st)

        def reweight(stage):
            return main.exmc_hip_smc_reweight(compiled.device, co, R, d, stage, q.data_ptr(), lp.data_ptr(), st)

        def mutate():
            return L.exmc_hip_smc_mutate(h, co, R, q.data_ptr(), lp.data_ptr(), words.data_ptr(), st)
    _ordered_after_torch(q)
    compiled.check(init())
    mutate_ms = 0.0
    for stage in range(S + 1):       # the reweight at stage == max_stages only closes the histories
        _lib.check(reweight(stage), main)
        if int(t["active_count"].cpu()[0]) == 0:
            break
        compiled.check(mutate())
        mutate_ms += compiled.last_kernel_ms
    torch.cuda.synchronize(dev)
    host = {k: v.cpu().numpy() for k, v in t.items()}
    extra = {}
    if bridged:
        extra = dict(logb=lb.cpu().numpy().reshape(R, N), log_evidence=le.cpu().numpy(),
                     log_evidence_steps=np.ascontiguousarray(les.cpu().numpy().T))
    return dict(extra, particles=np.ascontiguousarray(q.cpu().numpy().T).reshape(R, N, d),
                logp=lp.cpu().numpy().reshape(R, N), betas=np.ascontiguousarray(host["betas"].T),
                ess_history=np.ascontiguousarray(host["ess_history"].T),
                acceptance_rates=np.ascontiguousarray(host["acceptance_rates"].T), num_stages=host["num_stages"],
                status=host["status"], kernel_ms=mutate_ms, mutate_ms=mutate_ms)


def _sample(ir_or_compiled, opts, num_runs, raw_fn):
    o = _validate(opts, num_runs)        # before the library is touched
    from . import sampler
    compiled = ir_or_compiled if isinstance(ir_or_compiled, sampler.Compiled) else \
        sampler.Compiled(ir_or_compiled, device=o.get("device", 0))
    raw = raw_fn(compiled, o, num_runs)
    traces, infos = [], []
    for r in range(int(num_runs)):
        n = int(raw["num_stages"][r])
        traces.append(sampler._build_trace(compiled.spec, raw["particles"][r]))
        infos.append(dict(num_stages=n, betas=[float(x) for x in raw["betas"][r, :n]],
                          ess_history=[float(x) for x in raw["ess_history"][r, :n]],
                          acceptance_rates=[float(x) for x in raw["acceptance_rates"][r, :n]],
                          status=int(raw["status"][r])))
        if "log_evidence" in raw:
            infos[-1].update(log_evidence=float(raw["log_evidence"][r]),
                             log_evidence_steps=[float(x) for x in raw["log_evidence_steps"][r, :n]])
    if int(num_runs) == 1:
        return traces[0], infos[0]
    return traces, infos


def sample(ir_or_compiled, opts=None, num_runs=1):
    """Exmc.SMC.sample/2; with num_runs > 1 a batch of runs: lists of traces and infos."""
    return _sample(ir_or_compiled, opts, num_runs, sample_raw)


def sample_bridged(ir_or_compiled, opts=None, num_runs=1, base=None):
    """Bridged SMC: `sample` with the start divided out of the weights; info also holds log_evidence, the
    estimate of log p(y), and log_evidence_steps. base: None, (mu, sigma) or a dict with mu and sigma or
    log_sigma, in the unconstrained kernel order."""
    if base is not None and not isinstance(base, dict):
        mu, sigma = base                 # a malformed base fails before the library is touched
    return _sample(ir_or_compiled, opts, num_runs, lambda c, o, n: sample_bridged_raw(c, o, n, base))


def pooled_log_evidence(infos):
    """The log of the mean of exp(log_evidence) over the runs of a batch (the evidence estimate of a run is
    unbiased, its logarithm is not): on the host. `infos` is a list of infos, one info, or an array."""
    if isinstance(infos, dict):
        infos = [infos]
    le = np.array([i["log_evidence"] if isinstance(i, dict) else i for i in infos], dtype=np.float64).reshape(-1)
    m = float(np.max(le))
    if not math.isfinite(m):
        return m
    return m + math.log(float(np.mean(np.exp(le - m))))
