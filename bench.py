#!/usr/bin/env python
"""bench.py -- q-KG gradient evaluations / s on BASELINE.json's headline configuration (C3: n=1000, d=8, q=4, 10k MC).

    python bench.py --gpus N --steps K --warmup W

N > 1 runs one rank per GPU over RCCL: either the driver launches this file under `python -m torch.distributed.run
--nproc-per-node N ...` (RANK / LOCAL_RANK / WORLD_SIZE in the environment), or -- when it is called plainly -- bench.py
re-launches ITSELF that way (127.0.0.1 rendezvous on a free port) and relays rank 0's JSON line.

A "step" is one pass of the hot path over one batch.  Round 3: the batch is BASELINE.json's C4 job itself -- 64 multistart
restarts (independent points_to_sample sets, same GP / discrete set / normal table: the axis of
ComputeKGOptimalPointsToSampleViaMultistartGradientDescent, gpp_knowledge_gradient_optimization.hpp:860-935) of the C3
evaluation, SHARDED over the ranks: 64 / N q-KG value+gradient evaluations per GPU per step in ONE moe_kg_batch call, then --
N > 1 -- ONE all_gather of the (KG, grad KG) rows.  Total work per step is fixed ("scaling": "strong"); at N = 1 a step is the
whole C4 job on one GPU (~40 ms), at N = 8 it is C4 as BASELINE.json states it (8 restarts per GPU).  `--restarts R` fixes
the per-GPU count instead ("weak").  `--shard mc` splits the 10k MC samples of each evaluation across ranks with one
all_reduce per evaluation (strong scaling of a single evaluation); at N > 1 the default run times that mode too, AFTER the K
timed steps, and reports it as the extra object "mc_shard".
`value` = evaluations all ranks completed / max-over-ranks wall time of the K timed steps; the GP (K factor, K^-1 y) is
resident in HBM before the timed region; per-call host inputs are the q x d query points, the P discrete points and the
normal table (PCIe-inclusive by construction -- see DESIGN.md).

First contact with a multi-GPU node (cornell_moe_amd/dist.py: bring_up): the control plane is a gloo group; RCCL is tried in
a throw-away child process per rank first (bring-up + one checked all_reduce, 60 s limit) and only used when every rank's
child passed -- otherwise the same measurement runs with its collectives on gloo and says so ("rccl_ranks": 0,
"fallback": ...).  If not even the rendezvous works, rank 0 drives all N devices in-process through the C ABI
(moe_kg_batch_multi) and the other ranks exit.  After the timed region rank 0 recomputes every restart on its own GPU and
reports the largest difference to the gathered results ("determinism"; restarts are bit-identical, MC shards <= 1e-12).

A plain run does only what the headline line needs: set-up, warm-up, the K timed steps, the result line (its `roofline` read
from the timed steps' own kernel times, with the committed HBM traffic beside them).  Everything else it can measure or check --
the determinism recompute, the batch-1 / batch-8 / MC-sharded extras, the in-run PMC passes, the covariance-build and K(X,X)
probes, the sustained FP64 rate, the other BASELINE configurations and the CPU reference baseline -- runs only with `--full`
(the `--no-*` options then drop single parts of it).  `--dump-outputs DIR` writes what the last timed step returned to its
caller (KG values and gradients of every restart; a suggestion's point and KG) as DIR/<name>.npy in float64; the inputs are
seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_TBS = 8.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP64_PEAK_TFLOPS = 78.6   # MI355X FP64: vector == matrix (MFMA) dense peak, 256 CU x 4 SIMD x 32 flop/clk x 2.4 GHz


def cpu_baseline(w, best, sample_mc, log, budget_s=60.0):
    """The reference CPU path (oracle/_ref, the unmodified C++) timed on this box's host cores on bounded samples of the
    same workload: (1) ONE core, ComputeGradKnowledgeGradient (a single evaluation is inherently one thread in the
    reference: its MC loop is serial); (2) a THREAD SWEEP the way the reference itself parallelises -- T independent evaluations
    under OpenMP, one State + RNG per thread (gpp_optimization.hpp:1472-1546) -- at T in {8, 32, 64, 128, 256} (up to the core count),
    keeping the best throughput.
    r5: an evaluation costs T(M) = T0 + M t_s -- T0 the state set-up and the (N + m)^3 / 3 re-factorisation of
    the fantasy GP (gpp_math.cpp:1720-1747), paid once per evaluation whatever M -- so every thread count is timed at TWO sample
    counts and the line through them is read at M = 10 000 (as cpu_baseline_c5 does); scaling one short run linearly in M multiplied
    T0 by 25 and made the CPU look 10-20 % slower than it is.  `value` is the BEST CPU throughput found (what the >= 10x target is
    judged against); `cores` the threads it used."""
    try:
        from oracle import ref
        if ref.available():
            ncores = ref.num_procs()
            gp = ref.RefGP(1, w.alpha, w.lengths, w.X, w.y, w.noise, ())
            t_begin = time.time()

            def fit(walls, counts):
                t_s = (walls[1] - walls[0]) / float(counts[1] - counts[0])
                t0 = max(walls[0] - counts[0] * t_s, 0.0)
                return t0, t_s, t0 + w.M * t_s

            one_counts = (max(sample_mc, 100), 4 * max(sample_mc, 100))
            one_walls = []
            for mc in one_counts:
                r1 = gp.kg(w.inner_gd, w.bounds, w.discrete, w.Xq, None, mc, best, w.kg_normals[: (mc + 1) // 2])
                one_walls.append(r1["seconds"][0] + r1["seconds"][1])
            t0_1, ts_1, full_1 = fit(one_walls, one_counts)
            one_core = 1.0 / full_1
            sweep = [{"threads": 1, "evals_per_s": one_core, "sample_mc": list(one_counts), "wall_s": one_walls, "T0_s": t0_1,
                      "per_sample_s": ts_1, "linear_in_M_evals_per_s": 1.0 / (one_walls[1] * w.M / float(one_counts[1]))}]
            for T in (8, 32, 64, 128, 256):
                if T > ncores or time.time() - t_begin > budget_s:
                    break
                counts = (max(sample_mc // 4, 50), max(sample_mc // 4, 50) * 3) if T <= 64 else (max(sample_mc // 8, 50), max(sample_mc // 8, 50) * 3)
                Xq_all = np.ascontiguousarray(w.Xq_restarts[np.arange(T) % len(w.Xq_restarts)])
                walls = []
                for mc in counts:
                    _, _, wall = gp.kg_grad_batch(w.inner_gd, w.bounds, w.discrete, Xq_all, mc, best, w.kg_normals[: (mc + 1) // 2], T)
                    walls.append(wall)
                t0, t_s, full = fit(walls, counts)
                sweep.append({"threads": T, "evals_per_s": T / full, "sample_mc": list(counts), "wall_s": walls, "T0_s": t0,
                              "per_sample_s": t_s, "linear_in_M_evals_per_s": T / (walls[1] * w.M / float(counts[1]))})
            top = max(sweep, key=lambda e: e["evals_per_s"])
            # r6: the best point of the sweep measured a SECOND time (its spread says how far to trust the sweep),
            # and what the host looks like to this process -- the sweep usually peaks far below the core count: every thread's State
            # owns a copy of the fantasy GP and streams its (N + m)^2 factor (8 MB at C3) through two triangular sweeps per MC sample
            # (gpp_math.cpp:531-551), so beyond a few dozen threads the run is bound by the sockets' memory bandwidth and the shared
            # L3, and threads placed across NUMA nodes (no OMP_PROC_BIND in the reference's own drivers) make it worse, not better
            repeat = None
            if top["threads"] > 1 and time.time() - t_begin <= 1.5 * budget_s:
                T = top["threads"]
                Xq_all = np.ascontiguousarray(w.Xq_restarts[np.arange(T) % len(w.Xq_restarts)])
                walls = [gp.kg_grad_batch(w.inner_gd, w.bounds, w.discrete, Xq_all, mc, best, w.kg_normals[: (mc + 1) // 2], T)[2]
                         for mc in top["sample_mc"]]
                repeat = {"threads": T, "evals_per_s": T / fit(walls, top["sample_mc"])[2], "wall_s": walls}
            host = {"online_cpus": ncores, "affinity_cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,
                    "numa_nodes": len([n_ for n_ in os.listdir("/sys/devices/system/node") if n_.startswith("node")])
                    if os.path.isdir("/sys/devices/system/node") else None,
                    "omp_env": {k: os.environ[k] for k in ("OMP_NUM_THREADS", "OMP_PROC_BIND", "OMP_PLACES", "GOMP_CPU_AFFINITY") if k in os.environ}}
            return {"value": top["evals_per_s"], "unit": "evals/s", "cores": top["threads"], "kind": "reference",
                    "host_cores": ncores, "one_core_evals_per_s": one_core, "thread_sweep": sweep, "repeat_of_best": repeat, "host": host,
                    "why_the_sweep_peaks_below_the_core_count": "one 8 MB factor per thread streamed twice per MC sample: memory-bandwidth / "
                                                                "L3 bound beyond a few dozen threads; threads unpinned, as in the reference's drivers",
                    "model": "T(M) = T0 + M t_s per evaluation, from two sample counts per thread count, read at M = %d" % w.M,
                    "sample": "1 core: ComputeGradKnowledgeGradient at n=%d d=%d q=%d with %d and %d of the %d MC samples "
                              "(%.1f + %.1f s); sweep: T independent evaluations under OpenMP (one per thread) with two sample counts "
                              "each (%s); value = best throughput of the sweep (at %d threads); `linear_in_M_evals_per_s` is what "
                              "rounds 1-4 reported (one run scaled linearly in M)"
                              % (w.n, w.d, w.q, one_counts[0], one_counts[1], w.M, one_walls[0], one_walls[1],
                                 ", ".join("T=%d: %d/%d" % (e["threads"], e["sample_mc"][0], e["sample_mc"][1]) for e in sweep[1:]),
                                 top["threads"])}
    except Exception as e:  # pragma: no cover
        log("cpu_baseline: reference unavailable (%s); using the C port" % e)
    from oracle import orc
    gp = orc.OrcGP(1, w.alpha, w.lengths, w.X, w.y, w.noise, ())
    t0 = time.time()
    gp.kg(w.inner_gd, w.bounds, w.discrete, w.Xq, None, sample_mc, best, w.kg_normals[: (sample_mc + 1) // 2])
    wall = time.time() - t0
    return {"value": 1.0 / (wall * w.M / float(sample_mc)), "unit": "evals/s", "cores": 1, "kind": "port",
            "sample": "one orc_kg value+gradient at %d of %d MC samples, wall %.2f s, scaled linearly in M" % (sample_mc, w.M, wall)}


def cpu_baseline_c5(w, log):
    """C5 (d-KG, n=2000, g=3: N=8000, M=20 000) takes the reference hours per evaluation on one core, so its time is
    EXTRAPOLATED: the unmodified reference (oracle/_ref) is timed at n in {250, 500, 1000} with two small sample
    counts each, which separates the per-sample cost t_s(N) (two (N+m)^2 triangular sweeps + the inner optimisation's passes
    over N entries: fitted as a N + b N^2) from the per-evaluation cost T_0(N) (state set-up and the (N+m)^3/3 refactorisation
    of the fantasy GP: fitted as c N^2 + e N^3); then T(C5) = T_0(8000) + 20 000 t_s(8000)."""
    from cornell_moe_amd.workloads import make_workload
    from oracle import ref
    if not ref.available():
        return {"value": None, "unit": "evals/s", "cores": 1, "kind": "reference", "sample": "oracle/_ref not built"}
    M1, M2 = 8, 24
    Ns, ts, T0 = [], [], []
    rows = []
    for n in (250, 500, 1000):
        ww = make_workload("C5", n=n, M=M2)
        gp = ref.RefGP(1, ww.alpha, ww.lengths, ww.X, ww.y, ww.noise, list(ww.derivs))
        best = float(gp.additional_mean(ww.discrete).min())
        tt = []
        for M in (M1, M2):
            r = gp.kg(ww.inner_gd, ww.bounds, ww.discrete, ww.Xq, None, M, best, ww.kg_normals[: (M + 1) // 2])
            tt.append(r["seconds"][0] + r["seconds"][1])
        per_sample = (tt[1] - tt[0]) / float(M2 - M1)
        fixed = tt[0] - M1 * per_sample
        N = n * (1 + ww.g)
        Ns.append(float(N))
        ts.append(per_sample)
        T0.append(fixed)
        rows.append({"n": n, "N": N, "seconds_M%d" % M1: tt[0], "seconds_M%d" % M2: tt[1], "per_sample_s": per_sample, "fixed_s": fixed})
        log("cpu_baseline C5: n=%d N=%d: %.2f s at M=%d, %.2f s at M=%d" % (n, N, tt[0], M1, tt[1], M2))
    Ns = np.array(Ns)
    # non-negative least squares: with three noisy timings an unconstrained fit can return a negative coefficient, which at
    # N = 8000 (twice the largest measured size) may even turn the extrapolated time negative
    try:
        from scipy.optimize import nnls
        ab = nnls(np.c_[Ns, Ns ** 2], np.maximum(np.array(ts), 0.0))[0]
        ce = nnls(np.c_[Ns ** 2, Ns ** 3], np.maximum(np.array(T0), 0.0))[0]
    except ImportError:  # leading terms through the largest size
        ab = np.array([0.0, max(ts[-1], 0.0) / Ns[-1] ** 2])
        ce = np.array([0.0, max(T0[-1], 0.0) / Ns[-1] ** 3])
    Nc = float(w.n * (1 + w.g))
    t_s = float(ab[0] * Nc + ab[1] * Nc ** 2)
    t_0 = float(ce[0] * Nc ** 2 + ce[1] * Nc ** 3)
    total = t_0 + w.M * t_s
    return {"value": 1.0 / total, "unit": "evals/s", "cores": 1, "kind": "reference", "extrapolated_seconds_per_eval": total,
            "model": "T = T0(N) + M t_s(N); t_s = a N + b N^2, T0 = c N^2 + e N^3 (non-negative least squares over the three sizes)",
            "fit": {"a": float(ab[0]), "b": float(ab[1]), "c": float(ce[0]), "e": float(ce[1]), "t_s_at_C5": t_s, "T0_at_C5": t_0},
            "measurements": rows,
            "sample": "reference ComputeGradKnowledgeGradient (1 core) at n = 250, 500, 1000 (N = 1000, 2000, 4000) with %d and %d MC "
                      "samples, extrapolated to N = %d, M = %d" % (M1, M2, int(Nc), w.M)}


def dump_outputs(dirname, **arrays):
    """--dump-outputs: one DIR/<name>.npy (float64) per array the timed path returned in its last step."""
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def committed_traffic():
    """HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/hbm_traffic.json)."""
    try:
        with open(os.path.join(ROOT, "profiles", "hbm_traffic.json")) as fh:
            return json.load(fh)
    except Exception:
        return {}


def measure_traffic(config, restarts, log, timeout_s=180, passes=None):
    """HBM bytes per launch AND executed FP64 wave-instructions per launch of the reported kernels, measured NOW: three rocprofv3
    passes (FETCH_SIZE; WRITE_SIZE; SQ_INSTS_VALU_{FMA,ADD,MUL,TRANS}_F64 -- each in its own --pmc run with --kernel-trace only,
    as MI355X_MICROARCH.md prescribes; FETCH_SIZE doubled for gfx950) over tools/prof_kg.py -- the same batched evaluation this
    file times -- reduced by tools/hbm_traffic.py.  Returns (dict kernel -> dict of per-launch figures, source string); falls
    back to the committed measurement when the profiler is missing."""
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    tmp = tempfile.mkdtemp(prefix="moe_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    try:
        for tag, ctrs in (("fetch", ["FETCH_SIZE"]), ("write", ["WRITE_SIZE"]),
                          ("fp64", ["SQ_INSTS_VALU_FMA_F64", "SQ_INSTS_VALU_ADD_F64", "SQ_INSTS_VALU_MUL_F64", "SQ_INSTS_VALU_TRANS_F64"]),
                          # r4: the clock the kernel actually ran at and how busy its vector ALUs were, IN the kernel
                          ("clock", ["GRBM_GUI_ACTIVE", "GRBM_COUNT"]),
                          ("busy", ["SQ_BUSY_CYCLES", "SQ_WAVE_CYCLES", "SQ_ACTIVE_INST_VALU", "SQ_INST_CYCLES_SALU"]),
                          ("insts", ["SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"])):
            if passes is not None and tag not in passes:
                continue
            cmd = [exe, "--kernel-trace", "--pmc"] + ctrs + ["--output-format", "csv", "-d", os.path.join(tmp, tag), "-o", "p",
                   "--", sys.executable, os.path.join(ROOT, "tools", "prof_kg.py"), config, str(restarts), "2"]
            try:
                # (rocprofv3 has been seen to die in its own teardown AFTER writing its tables: the exit code is not the criterion,
                #  the counter table is)
                subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s, check=False)
                import glob
                if not glob.glob(os.path.join(tmp, tag, "**", "*counter_collection.csv"), recursive=True):
                    raise RuntimeError("no counter table written")
            except Exception as e:  # the FP64 pass is an extra: keep the traffic passes' result if only it fails
                if tag in ("fetch", "write"):
                    raise
                log("measure_traffic: %s counter pass failed (%s)" % (tag, type(e).__name__))
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hbm_traffic.py"), tmp], stdout=subprocess.PIPE,
                             universal_newlines=True, timeout=60, check=True)
        data = json.loads(res.stdout.strip().splitlines()[-1])
        if not any(k.startswith("kg_mc") for k in data):
            return None, "rocprofv3 ran but reported no kg_mc kernel rows"
        data["evals_per_launch"] = restarts
        return data, "rocprofv3 --pmc passes (FETCH_SIZE | WRITE_SIZE | SQ_INSTS_VALU_*_F64) run by this bench.py invocation"
    except Exception as e:  # pragma: no cover
        log("measure_traffic failed: %s" % e)
        return None, "in-run PMC passes failed (%s)" % type(e).__name__
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def self_launch(args_list, n, script=None):
    """`python bench.py --gpus N` called plainly: re-launch under torch.distributed.run, one rank per GPU, relay the output.
    (`script` is a test hook: tests/test_host_logic.py drives this launcher with a gloo stand-in.)"""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), MOE_BENCH_SELF_LAUNCHED="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), script or os.path.abspath(__file__)] + args_list
    return subprocess.call(cmd, env=env)


def suggest_problem(kind):
    """The production regime of the reference's own example (examples/main.py:90-142, examples/bayesian_optimization.py:60-88): ONE
    q-KG suggestion = multistart_knowledge_gradient_mcmc_optimization over an ensemble of 16 hyper-parameter samples -- 200
    Latin-hypercube starts, the best 20 kept, gradient ascent of 50 steps x 2 restarts (gamma 0.7, max_relative_change 0.5), every KG
    evaluation with 2^7 Monte-Carlo samples whose inner optimisations run 6 steps; q = 4.  `suggest`: Branin (d = 2) with n = 30 points;
    `suggest_c3`: the same optimiser on a GP of the headline size (n = 1000, d = 8).  Synthetic hyper-parameter samples (log-normal
    around the data's scale), 10 shared discretised points + 1 per member (main.py:170-198)."""
    rng = np.random.default_rng(20250 + (0 if kind == "suggest" else 1))
    if kind == "suggest":
        d, n = 2, 30
        lo, hi = np.array([0.0, -5.0]), np.array([15.0, 15.0])
        X = lo + (hi - lo) * rng.uniform(size=(n, d))
        a, b, c, r, sdash, t = 1.0, 5.1 / (4 * np.pi ** 2), 5.0 / np.pi, 6.0, 10.0, 1.0 / (8 * np.pi)
        y = (a * (X[:, 1] - b * X[:, 0] ** 2 + c * X[:, 0] - r) ** 2 + sdash * (1 - t) * np.cos(X[:, 0]) + sdash)[:, None]
        base_len = np.array([4.0, 6.0])
    else:
        from cornell_moe_amd.workloads import make_workload
        w = make_workload("C3")
        d, n = w.d, w.n
        lo, hi = np.asarray(w.bounds)[0::2], np.asarray(w.bounds)[1::2]
        X, y = w.X, w.y[:, :1]
        base_len = np.asarray(w.lengths)
    num_mcmc, q, M, P = 16, 4, 128, 11
    alpha0 = float(np.var(y)) if kind == "suggest" else float(w.alpha)
    hypers = np.c_[alpha0 * np.exp(0.3 * rng.standard_normal(num_mcmc)), base_len * np.exp(0.2 * rng.standard_normal((num_mcmc, d)))]
    noises = np.full((num_mcmc, 1), 1e-4 * alpha0)
    shared = lo + (hi - lo) * rng.uniform(size=(P - 1, d))
    discrete_all = np.stack([np.vstack([shared, lo + (hi - lo) * rng.uniform(size=(1, d))]) for _ in range(num_mcmc)])
    bounds = np.c_[lo, hi].reshape(-1)
    return dict(kind=kind, d=d, n=n, q=q, M=M, P=P, num_mcmc=num_mcmc, X=np.ascontiguousarray(X), y=np.ascontiguousarray(y),
                hypers=hypers, noises=noises, discrete_all=discrete_all, bounds=bounds,
                outer_gd=(200, 50, 2, 4, 0.7, 1.0, 0.5, 1.0e-10), inner_gd=(1, 6, 1, 3, 0.0, 1.0, 0.1, 1.0e-10),
                uniform_seed=314, normal_seed=271)


def run_suggest(args, rank, local_rank, world, comm, log):
    """bench.py --config suggest | suggest_c3 (r5): the wall time of ONE whole suggestion.  N = 1: moe_kg_mcmc_multistart
    on one GPU; N > 1: the ensemble's members dealt to the ranks (moe_kg_mcmc_multistart_comm, one all-gather per optimiser step over
    the data-plane group).  A step = one suggestion; `value` = seconds per suggestion (max over ranks).  Next to it the reference's
    ComputeKGMCMCOptimalPointsToSampleViaMultistartGradientDescent on the host cores with the reference's own thread count (20;
    examples/bayesian_optimization.py:84) -- in full for `suggest`, on a bounded sample (fewer GD steps, scaled by the step count of
    the device run) for `suggest_c3` -- and the per-step timeline of the device run (moe_multistart_trace)."""
    import torch
    from cornell_moe_amd import api as mapi, dist as mdist
    pb = suggest_problem(args.config)
    d, q, M, nm = pb["d"], pb["q"], pb["M"], pb["num_mcmc"]
    members = mdist.shard_members(nm, rank, world) if world > 1 else None
    t_build = time.perf_counter()
    G = mapi.DeviceGPMCMC(pb["hypers"], pb["noises"], pb["X"], pb["y"], (), device=local_rank, members=members)
    build_s = time.perf_counter() - t_build
    # best posterior mean over each member's discretised set (knowledge_gradient_mcmc.py: best_so_far per GP)
    best_local = np.array([float(g.additional_mean(pb["discrete_all"][i]).min()) for g, i in zip(G.gps, G.members)])
    best_all = np.zeros(nm)
    best_all[G.members] = best_local
    if world > 1:
        allb = comm.gather_floats(list(best_all))
        best_all = np.sum(np.array(allb), axis=0)
    starts = np.stack([mapi.latin_hypercube(pb["uniform_seed"] + k, pb["bounds"], pb["outer_gd"][0]) for k in range(q)], axis=1)
    normals = mapi.normal_draws(pb["normal_seed"], ((M + 1) // 2) * q)
    ex = mdist.make_exchange(comm, local_rank) if world > 1 else None   # (RCCL data plane: the library's native communicator, r6)

    def suggestion():
        return G.kg_multistart(pb["outer_gd"], pb["inner_gd"], pb["bounds"], pb["discrete_all"], starts, None, M, best_all, normals,
                               comm=ex)

    def fence():
        torch.cuda.synchronize()
        comm.barrier()

    for _ in range(max(args.warmup, 1) if args.warmup_set else 1):
        pt, val, found = suggestion()
    fence()
    if ex is not None:
        ex.calls, ex.doubles, ex.seconds = 0, 0, 0.0
    steps = args.steps if args.steps_set else 3
    t0 = time.perf_counter()
    for _ in range(steps):
        pt, val, found = suggestion()
    local_elapsed = time.perf_counter() - t0
    fence()
    elapsed = comm.max_over_ranks(time.perf_counter() - t0)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, best_point=pt, best_kg=np.array([val]))
    trace = mapi.multistart_trace()
    pts_all = comm.gather_floats(list(pt.ravel()) + [val])
    if rank != 0:
        comm.close()
        return
    sec = elapsed / steps
    grads = trace[trace[:, 0] == 1]
    vals = trace[trace[:, 0] == 0]
    out = {
        "metric": "q-KG-MCMC suggestion wall time (%s)" % ("examples/main.py settings: Branin n=30, 16 GPs, 200 starts -> 20, 50 steps x 2 restarts, "
                                                          "M=128, q=4" if pb["kind"] == "suggest" else
                                                          "the same optimiser on a GP of the headline size n=1000, d=8, q=4, 16 GPs, M=128"),
        "value": sec, "unit": "s per suggestion", "n_gpus": world, "steps": steps, "warmup": 1, "ms_per_step": 1e3 * sec,
        "higher_is_better": False, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "%s: multistart_knowledge_gradient_mcmc_optimization, n=%d d=%d q=%d num_mcmc=%d M=%d P=%d, outer GD %s, inner GD %s; "
                               "%s" % (pb["kind"], pb["n"], d, q, nm, M, pb["P"], pb["outer_gd"], pb["inner_gd"],
                                       "one GPU" if world == 1 else "members dealt to %d ranks, one all-gather per optimiser step" % world),
                   "shard": "members" if world > 1 else "none"},
        "rccl_ranks": comm.rccl_ranks, "collective_backend": comm.backend, "fallback": comm.fallback,
        "found": bool(found), "best_kg": float(val), "best_point": [float(v) for v in pt.ravel()],
        "all_ranks_agree": bool(all(r == pts_all[0] for r in pts_all)),
        "ensemble_build_s": build_s,
        "timeline": {"batched_evaluations": int(len(trace)), "gradient_steps": int(len(grads)),
                     "ms_per_gradient_step": {"mean": float(grads[:, 2].mean()) if len(grads) else None,
                                              "median": float(np.median(grads[:, 2])) if len(grads) else None,
                                              "first": float(grads[0, 2]) if len(grads) else None,
                                              "last": float(grads[-1, 2]) if len(grads) else None},
                     "live_restarts_per_step": {"first": int(grads[0, 1]) if len(grads) else None, "last": int(grads[-1, 1]) if len(grads) else None,
                                                "mean": float(grads[:, 1].mean()) if len(grads) else None},
                     "value_passes": [{"items": int(r[1]), "ms": float(r[2])} for r in vals],
                     "ms_in_gradient_steps": float(grads[:, 2].sum()), "ms_in_value_passes": float(vals[:, 2].sum()),
                     "source": "moe_multistart_trace of the last timed suggestion (rank 0): wall time of every batched evaluation the optimiser "
                               "issued, exchange included"},
    }
    if ex is not None:
        out["exchange"] = {"provider": type(ex).__name__, "calls_per_suggestion": ex.calls / float(steps), "doubles_per_call": ex.doubles / float(max(ex.calls, 1)),
                           "ms_per_call": 1e3 * ex.seconds / max(ex.calls, 1), "s_per_suggestion": ex.seconds / steps}
    if args.full and not args.no_cpu_baseline and world == 1:
        try:
            from oracle import ref
            assert ref.available() and hasattr(ref.lib(), "ref_kg_mcmc_multistart_mt")
            ncores = ref.num_procs()
            R = ref.RefGPMCMC(pb["hypers"], pb["noises"], pb["X"], pb["y"], [])
            T = min(20, ncores)   # the reference's own setting (examples/bayesian_optimization.py:84: max_num_threads=20)
            if pb["kind"] == "suggest":
                rp, rfound, wall = R.kg_multistart_mt(pb["outer_gd"], pb["inner_gd"], pb["bounds"], pb["discrete_all"], starts, None, M, best_all,
                                                      pb["normal_seed"], T)
                note = "the reference's driver in full, %d OpenMP threads" % T
                ref_pt = [float(v) for v in rp.ravel()]
            else:
                # bounded: 2 GD steps x 1 restart instead of 50 x 2 -- the 200-start value pass and the closing value pass in full -- then
                # the gradient steps scaled to the number the device run took (restarts that stop early stop early in both)
                # (at this size one KG-MCMC evaluation costs the reference seconds -- 16 re-factorisations of an (N + m)^2 matrix -- so the
                #  value passes are timed on 40 of the 200 starts (40 + 20 evaluations instead of 200 + 20) and scaled by the count)
                sub = np.ascontiguousarray(starts[:40])
                none = (40, 1, 0, 4, 0.7, 1.0, 0.5, 1.0e-10)    # max_num_restarts = 0: the two value passes only
                _, _, w_vals = R.kg_multistart_mt(none, pb["inner_gd"], pb["bounds"], pb["discrete_all"], sub, None, M, best_all,
                                                  pb["normal_seed"], T)
                short = (40, 3, 1, 4, 0.7, 1.0, 0.5, 1.0e-10)   # + 3 gradient steps of the 20 kept restarts
                _, _, w_short = R.kg_multistart_mt(short, pb["inner_gd"], pb["bounds"], pb["discrete_all"], sub, None, M, best_all,
                                                   pb["normal_seed"], T)
                per_step = max(w_short - w_vals, 0.0) / 3.0
                vals_full = w_vals * (200 + 20) / float(40 + 20)
                wall = vals_full + per_step * len(grads)
                note = ("EXTRAPOLATED: value passes %.1f s (timed on 40 + 20 evaluations: %.1f s, scaled to 200 + 20) + %d gradient steps x "
                        "%.2f s per step of 20 restarts (from a 3-step run), %d OpenMP threads" % (vals_full, w_vals, len(grads), per_step, T))
                ref_pt = None
            out["cpu_baseline"] = {"value": wall, "unit": "s per suggestion", "cores": T, "host_cores": ncores, "kind": "reference",
                                   "sample": note, "best_point": ref_pt}
            out["speedup_vs_cpu"] = wall / sec
            if ref_pt is not None:
                out["max_abs_diff_vs_reference_point"] = float(np.abs(np.array(ref_pt) - pt.ravel()).max())
        except Exception as e:  # pragma: no cover
            log("suggest: reference timing unavailable (%s: %s)" % (type(e).__name__, e))
    print(json.dumps(out), flush=True)
    comm.close()


def side_configs(local_rank, log, c5_traffic=True):
    """r6: every other BASELINE.json configuration measured by the DEFAULT run, after the timed region, as a compact
    object -- C1 posterior queries (us), C2 q-EI value + gradient (us), C5 d-KG (evals/s, its MC phase against the FP64 peak with the
    device-counted passes, HBM traffic of the phase from an in-run PMC pass), one whole KG-MCMC suggestion (s) -- so that the driver's
    record of the headline line carries them.  Each entry is reproducible alone: `bench.py --config C5`, `--config suggest`,
    tools/latency.py."""
    import torch
    from cornell_moe_amd import api as mapi
    from cornell_moe_amd.api import DeviceGP
    from cornell_moe_amd.workloads import make_workload
    out = {}

    def timed(fn, reps, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    try:   # configs[0]: GP posterior mean / variance, n = 200, d = 2
        w = make_workload("C1")
        t0 = time.perf_counter()
        G = DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, device=local_rank)
        build_ms = 1e3 * (time.perf_counter() - t0)
        one, hundred = w.query[:1], w.query[:100]
        out["C1"] = {"workload": "posterior mean / variance, n=200 d=2 (the GP stays resident)", "gp_build_ms": build_ms,
                     "mean_1pt_us": 1e6 * timed(lambda: G.mean(one), 200), "var_1pt_us": 1e6 * timed(lambda: G.variance(one), 200),
                     "mean_100pts_us": 1e6 * timed(lambda: G.mean(hundred), 100), "var_100pts_us": 1e6 * timed(lambda: G.variance(hundred), 50)}
        G.close()
    except Exception as e:  # pragma: no cover
        out["C1"] = {"error": "%s: %s" % (type(e).__name__, e)}
    try:   # configs[1]: q-EI value + gradient, n = 500, d = 4, q = 2, 1k MC, one at a time
        w = make_workload("C2")
        G = DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, device=local_rank)
        best = float(w.y[:, 0].min())
        out["C2"] = {"workload": "q-EI, n=500 d=4 q=2 M=1000, one evaluation per call",
                     "value_grad_us": 1e6 * timed(lambda: G.ei(w.Xq, None, w.M, best, w.ei_normals), 200),
                     "value_only_us": 1e6 * timed(lambda: G.ei(w.Xq, None, w.M, best, w.ei_normals, want_grad=False), 200)}
        G.close()
    except Exception as e:  # pragma: no cover
        out["C2"] = {"error": "%s: %s" % (type(e).__name__, e)}
    try:   # configs[4]: d-KG, n = 2000, d = 12, q = 8, g = 3, 20k MC -- two evaluations per call, as `--config C5`
        w = make_workload("C5", num_restarts=2)
        t0 = time.perf_counter()
        G = DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, device=local_rank)
        build_ms = 1e3 * (time.perf_counter() - t0)
        best = float(G.additional_mean(w.discrete).min())
        call = lambda: G.kg_batch(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts, None, w.M, best, w.kg_normals)  # noqa: E731
        call()
        torch.cuda.synchronize()
        steps, ms_mc, vp, gp_ = 4, 0.0, 0, 0
        t0 = time.perf_counter()
        for _ in range(steps):
            r = call()
            km = G.last_kernel_ms()
            ms_mc += km["mc"]
            vp += r["mean_evals"]
            gp_ += r["grad_evals"]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        npts, f_val, f_grad = pass_flops(w)
        S, Gp = vp / float(2 * steps * w.M), gp_ / float(2 * steps * w.M)
        flops = w.M * npts * (S * f_val + Gp * f_grad)
        mc_ms = ms_mc / steps       # per evaluation (HIP events on the library's stream: sample pre-pass + weight table + MC kernel)
        kinfo = G.last_kernel_info()
        kname = {0: "kg_mc_kernel", 1: "kg_mc_block_kernel", 2: "kg_mc_stream_kernel"}[kinfo["variant"]]
        out["C5"] = {"workload": "d-KG value+gradient, n=2000 d=12 q=8 g=3 M=20000, 2 evaluations per call", "evals_per_s": 2 * steps / dt,
                     "gp_build_ms": build_ms, "mc_phase_ms_per_eval": mc_ms, "kernel": kname,
                     "frac": flops / (mc_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS, "bound": "fp64_valu", "peak_tflops": FP64_PEAK_TFLOPS,
                     "value_passes_per_sample": S, "grad_passes_per_sample": Gp,
                     "weight_table_bytes_per_eval": 8.0 * w.M * ((w.n + w.q + 63) // 64) * 64 * (1 + w.g), "traffic_bytes_per_eval": None}
        try:   # the same evaluations eight per call (a multistart's batch): the state's and the tail's triangular products read L^-1 once per CALL
            w8 = make_workload("C5", num_restarts=8)
            call8 = lambda: G.kg_batch(w8.inner_gd, w8.bounds, w8.discrete, w8.Xq_restarts, None, w8.M, best, w8.kg_normals)  # noqa: E731
            call8()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2):
                call8()
            torch.cuda.synchronize()
            out["C5"]["evals_per_s_at_8_per_call"] = 16.0 / (time.perf_counter() - t0)
        except Exception as e:  # pragma: no cover
            out["C5"]["evals_per_s_at_8_per_call"] = "%s: %s" % (type(e).__name__, e)
        G.close()
        if c5_traffic:
            pmc, src = measure_traffic("C5", 2, log, timeout_s=90, passes=("fetch", "write"))
            pk = (pmc or {}).get(kname) or {}
            if pk.get("hbm_bytes_per_launch") is not None:
                out["C5"]["traffic_bytes_per_eval"] = pk["hbm_bytes_per_launch"] / 2.0
                out["C5"]["traffic_over_table"] = out["C5"]["traffic_bytes_per_eval"] / out["C5"]["weight_table_bytes_per_eval"]
            out["C5"]["traffic_source"] = src + " (MC kernel alone; the table's own write is one table size more)"
    except Exception as e:  # pragma: no cover
        out["C5"] = {"error": "%s: %s" % (type(e).__name__, e)}
    try:   # the thing users invoke: one whole KG-MCMC suggestion (examples/main.py's settings), as `--config suggest`
        pb = suggest_problem("suggest")
        q, M, nm = pb["q"], pb["M"], pb["num_mcmc"]
        G = mapi.DeviceGPMCMC(pb["hypers"], pb["noises"], pb["X"], pb["y"], (), device=local_rank)
        best_all = np.array([float(g.additional_mean(pb["discrete_all"][i]).min()) for g, i in zip(G.gps, G.members)])
        starts = np.stack([mapi.latin_hypercube(pb["uniform_seed"] + k, pb["bounds"], pb["outer_gd"][0]) for k in range(q)], axis=1)
        normals = mapi.normal_draws(pb["normal_seed"], ((M + 1) // 2) * q)
        sug = lambda: G.kg_multistart(pb["outer_gd"], pb["inner_gd"], pb["bounds"], pb["discrete_all"], starts, None, M, best_all, normals)  # noqa: E731
        sec = timed(sug, 3, warm=1)
        out["suggest"] = {"workload": "one q-KG-MCMC suggestion: Branin n=30, 16 GPs, 200 starts -> 20, 50 steps x 2 restarts, M=128, q=4",
                          "s_per_suggestion": sec}
        st = mapi.ensemble_launch_stats()   # (r6: every kernel issued once for all members of the ensemble, csrc/launch.hpp)
        out["suggest"]["ensemble_launches"] = {"merged_evaluations": st[0], "member_by_member_evaluations": st[1],
                                               "launches_issued": st[2], "member_launches_they_stand_for": st[3]}
        del G
        pb = suggest_problem("suggest_c3")   # the same optimiser on an ensemble of GPs of the headline size (n = 1000, d = 8)
        G = mapi.DeviceGPMCMC(pb["hypers"], pb["noises"], pb["X"], pb["y"], (), device=local_rank)
        best_all = np.array([float(g.additional_mean(pb["discrete_all"][i]).min()) for g, i in zip(G.gps, G.members)])
        starts = np.stack([mapi.latin_hypercube(pb["uniform_seed"] + k, pb["bounds"], pb["outer_gd"][0]) for k in range(q)], axis=1)
        sug3 = lambda: G.kg_multistart(pb["outer_gd"], pb["inner_gd"], pb["bounds"], pb["discrete_all"], starts, None, M, best_all, normals)  # noqa: E731
        out["suggest_c3"] = {"workload": "the same suggestion on 16 GPs of the headline size (n=1000, d=8)", "s_per_suggestion": timed(sug3, 1, warm=1)}
    except Exception as e:  # pragma: no cover
        out.setdefault("suggest", {"error": "%s: %s" % (type(e).__name__, e)})
        out.setdefault("suggest_c3", {"error": "%s: %s" % (type(e).__name__, e)})
    return out


C4_RESTARTS = 64  # BASELINE.json configs[3]: "q-KG 64-multistart x 10k MC sharded across 8 x MI355X"


def pass_flops(w):
    """SURVEY 8(d) algorithmic flops of ONE posterior-mean pass of the inner optimisation over the n + u tabulated points:
    (value pass, value + gradient pass).  Without derivative observations a point is one covariance entry: 3d + 32 and 5d + 34
    flops (distance, sqrt, exp, Matern polynomial, accumulation).  With g observed derivatives the 1 + g entries of a POINT share
    one distance / sqrt / exp (r3: VERDICT r2 weak 3 -- counting (n+u)(1+g) full entries overstated the work 3x at C5); what a
    derivative slot adds is its weight's fma into the point's derivative sum (2 flops; 4 in a gradient pass, which also
    accumulates first * w_a), plus one fma (value) / the second-derivative coefficient and its fma (gradient) per point."""
    pts = w.n + w.q + w.p
    val = 3 * w.d + 32 + ((2 * w.g + 2) if w.g else 0)
    grad = 5 * w.d + 34 + ((4 * w.g + 6) if w.g else 0)
    return pts, val, grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--restarts", type=int, default=None,
                    help="independent KG evaluations per GPU per step (weak scaling); default: C3 -- 64 per STEP shared by the "
                         "ranks (the C4 job, strong scaling); C5 -- 2 per GPU")
    ap.add_argument("--shard", choices=["restarts", "mc"], default="restarts")
    ap.add_argument("--config", default="C3")
    ap.add_argument("--derivs", type=int, default=None,
                    help="observe the first G partial derivatives instead of the configuration's own list (C5's stretch point of "
                         "SURVEY 8(d): --config C5 --derivs 12 -> N = 26 000, m = 104)")
    ap.add_argument("--cpu-sample-mc", type=int, default=400)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-traffic", action="store_true", help="skip the in-run rocprofv3 PMC passes (HBM traffic, executed FP64)")
    ap.add_argument("--no-mc-shard", action="store_true", help="N > 1: skip the extra MC-sharded measurement")
    ap.add_argument("--no-batch1", action="store_true", help="skip the extra one-at-a-time (batch-1 latency) measurement")
    ap.add_argument("--no-extras", action="store_true", help="skip the extra roofline probes (K(X,X) builds, sustained FP64 rate)")
    ap.add_argument("--no-determinism", action="store_true",
                    help="skip the recompute-and-compare check (profiling runs: every kg_mc_kernel launch is then a timed step's)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every extra measurement and check (CPU baseline, determinism, batch-1, "
                         "MC shard, PMC passes, roofline probes, the other configurations); a plain run times the steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float64)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(sys.argv[1:], args.gpus))
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))

    def log(msg):
        if rank == 0:
            print("[bench] " + msg, file=sys.stderr, flush=True)

    import torch
    from cornell_moe_amd import _lib, api as mapi, dist as mdist
    from cornell_moe_amd.api import DeviceGP
    from cornell_moe_amd.workloads import make_workload

    _lib.load()
    _lib.require_gpu()
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    # MOE_BENCH_BACKEND=gloo is a test hook: it lets the N > 1 code path run with several ranks sharing ONE GPU (collectives
    # on host tensors); the measured configuration is always nccl (= RCCL), one rank per GPU.
    backend = os.environ.get("MOE_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend != "nccl" or os.environ.get("MOE_BENCH_SHARE_GPU") == "1":   # (second test hook: ranks share a GPU, RCCL still preferred)
        local_rank = local_rank % ndev
    elif ndev == 1 and local_rank > 0:
        # a launcher that narrows every rank's visibility to its own GPU (HIP_VISIBLE_DEVICES per process): the one visible
        # device IS this rank's
        print("[bench] rank %d: LOCAL_RANK=%d but one visible device -- using device 0" % (rank, local_rank), file=sys.stderr, flush=True)
        local_rank = 0
    torch.cuda.set_device(local_rank)

    # ---- process groups: gloo control plane, RCCL data plane behind a pre-flight (dist.bring_up) ----
    multi_fallback = None   # last resort: rank 0 drives all devices in-process through moe_kg_batch_multi
    try:
        comm = mdist.bring_up(rank, world, local_rank, prefer=backend, log=log)
    except Exception as e:  # not even the rendezvous came up
        if rank != 0:
            print("[bench] rank %d: process-group bring-up failed (%s); leaving the run to rank 0" % (rank, e), file=sys.stderr, flush=True)
            return
        multi_fallback = "process-group bring-up failed (%s: %s)" % (type(e).__name__, e)
        log("NO PROCESS GROUP -- %s; rank 0 drives %d device(s) in-process through moe_kg_batch_multi" % (multi_fallback, min(world, ndev)))
        comm = mdist.Comm(0, 1, "none", None, None, multi_fallback)

    if args.config in ("suggest", "suggest_c3"):
        args.steps_set = "--steps" in sys.argv
        args.warmup_set = "--warmup" in sys.argv
        return run_suggest(args, rank, local_rank, world, comm, log)

    strong = args.restarts is None and args.config in ("C3", "C4") and args.shard == "restarts"
    if strong:
        if C4_RESTARTS % world:
            raise SystemExit("the C4 job (64 restarts per step) does not divide over %d ranks; pass --restarts" % world)
        R = C4_RESTARTS // world
    else:
        R = args.restarts if args.restarts is not None else ((1 if args.derivs else 2) if args.config == "C5" else 8)
    w = make_workload(args.config, num_restarts=R * world,
                      derivs=None if args.derivs is None else tuple(range(args.derivs)))
    if multi_fallback is not None:
        devs = list(range(min(world, ndev)))
        gps = [DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, device=dv) for dv in devs]
        G = gps[0]
    else:
        G = DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, device=local_rank)
    best = float(G.additional_mean(w.discrete).min())  # knowledge_gradient.py:366-368
    my_restarts = w.Xq_restarts[rank * R:(rank + 1) * R] if multi_fallback is None else w.Xq_restarts
    cw = comm.world

    coll = {"s": 0.0, "n": 0}   # time inside the restart-gather of the timed steps

    def step(mode=None, restarts=None):
        mode = mode or args.shard
        if multi_fallback is not None and restarts is None:
            r = mapi.kg_batch_multi(gps, "restarts" if mode == "restarts" else "mc", w.inner_gd, w.bounds, w.discrete,
                                    w.Xq_restarts if mode == "restarts" else w.Xq_restarts[:R], None, w.M, best, w.kg_normals)
            return r["kg_sum"] / w.M, r["grad_sum"] / w.M, r
        if mode == "restarts":
            mine = my_restarts if restarts is None else restarts
            r = G.kg_batch(w.inner_gd, w.bounds, w.discrete, mine, None, w.M, best, w.kg_normals)
            kg = r["kg_sum"] / w.M
            grad = r["grad_sum"] / w.M
            if cw > 1 and restarts is None:
                idx = list(range(rank * R, (rank + 1) * R))
                tc = time.perf_counter()
                kg, grad = mdist.gather_restarts(idx, kg, grad, R * cw, group=comm.group, device=comm.device)
                coll["s"] += time.perf_counter() - tc   # host tensor -> (device) -> all_gather -> host: the step's whole exchange
                coll["n"] += 1
            return kg, grad, r
        first, count = mdist.shard_samples(w.M, rank, cw)
        Xm = w.Xq_restarts[:R] if restarts is None else restarts
        Rm = len(Xm)
        r = G.kg_batch(w.inner_gd, w.bounds, w.discrete, Xm, None, w.M, best, w.kg_normals, first_sample=first, num_local=count)
        kg, grad = r["kg_sum"], r["grad_sum"]
        if cw > 1:
            import torch.distributed as dist
            buf = torch.from_numpy(np.concatenate([kg[:, None], grad.reshape(Rm, -1)], axis=1))
            buf = buf.to(comm.device) if comm.device is not None else buf
            dist.all_reduce(buf, group=comm.group)
            out = buf.cpu().numpy()
            kg, grad = out[:, 0], out[:, 1:].reshape(grad.shape)
        return kg / w.M, grad / w.M, r

    def fence():
        torch.cuda.synchronize()
        comm.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    coll["s"], coll["n"] = 0.0, 0
    t0 = time.perf_counter()
    ms_mc = ms_cov = ms_tail = ms_state = 0.0
    val_passes = grad_passes = 0
    for _ in range(args.steps):
        kg, grad, r = step()
        km = G.last_kernel_ms()
        ms_mc += km["mc"]
        ms_cov += km["cov_build"]
        ms_tail += km["tail"]
        ms_state += km["state"]
        val_passes += r["mean_evals"]
        grad_passes += r["grad_evals"]
    local_elapsed = time.perf_counter() - t0     # this rank's own time for its K steps (before the closing barrier)
    coll_us = 1e6 * coll["s"] / coll["n"] if coll["n"] else 0.0
    fence()
    elapsed = comm.max_over_ranks(time.perf_counter() - t0)
    assert np.all(np.isfinite(kg)) and np.all(np.isfinite(grad))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, kg=kg, grad=grad)

    eff_world = world if multi_fallback is None else len(gps)
    if multi_fallback is not None:
        evals_per_step = len(w.Xq_restarts) if args.shard == "restarts" else R
    else:
        evals_per_step = R * world if args.shard == "restarts" else R
    total_evals = evals_per_step * args.steps
    value = total_evals / elapsed
    per_rank = [r[0] for r in comm.gather_floats([(R if multi_fallback is None else evals_per_step) * args.steps / local_elapsed])]

    # ---- extras, OUTSIDE the timed region of `value` ----
    extras = {}
    if cw > 1 and args.shard == "restarts":
        # per step, the slowest rank: it includes the wait for the slowest rank's compute (the gather is the step's only barrier),
        # so rank 0's own figure -- usually the smallest -- is reported next to it
        cmax = comm.max_over_ranks(coll_us)
        extras["collective_us_per_step"] = {"max_over_ranks": cmax, "rank0": coll_us,
                                            "what": "dist.gather_restarts: pack, host->device, all_gather of %d x %d doubles, device->host, unpack"
                                                    % (R, 2 + w.q * w.d)}
    if args.no_determinism or not args.full:
        pass
    elif cw > 1 and args.shard == "restarts":
        # cross-rank determinism: rank 0 recomputes EVERY restart of the last step on its own GPU in one call and
        # compares with what the ranks computed and gathered -- restarts are independent evaluations, so the results must be
        # bit-identical whatever the sharding
        if rank == 0:
            ra = G.kg_batch(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts, None, w.M, best, w.kg_normals)
            kg1, grad1 = ra["kg_sum"] / w.M, ra["grad_sum"] / w.M
            sc = max(float(np.abs(grad1).max()), float(np.abs(kg1).max()))
            dmax = max(float(np.abs(kg - kg1).max()), float(np.abs(grad - grad1).max())) / sc
            extras["determinism"] = {"max_rel_diff_vs_one_rank": dmax, "ok": bool(dmax <= 1e-12), "restarts": int(len(kg1)),
                                     "note": "all %d restarts recomputed by rank 0 alone vs the gathered per-rank results" % len(kg1)}
        fence()
    elif cw == 1 and multi_fallback is None and args.shard == "restarts" and R > 1:
        # N = 1: the same property across BATCHES -- the first restarts evaluated in a call of their own
        k = min(R, 4)
        rb = G.kg_batch(w.inner_gd, w.bounds, w.discrete, my_restarts[:k], None, w.M, best, w.kg_normals)
        sc = max(float(np.abs(grad).max()), float(np.abs(kg).max()))
        dmax = max(float(np.abs(rb["kg_sum"] / w.M - kg[:k]).max()), float(np.abs(rb["grad_sum"] / w.M - grad[:k]).max())) / sc
        extras["determinism"] = {"max_rel_diff_vs_separate_call": dmax, "ok": bool(dmax <= 1e-12), "restarts": k,
                                 "note": "the first %d restarts of the step evaluated in a call of their own" % k}
    if args.full and cw > 1 and args.shard == "restarts" and not args.no_mc_shard:
        # MC-sample sharding of ONE evaluation at a time (strong scaling of the single-evaluation latency): every rank takes an
        # even-aligned slice of the 10k samples, ONE all_reduce of 1 + q d doubles per evaluation
        one = w.Xq_restarts[:1]
        ksteps = max(10, args.steps)
        for _ in range(3):
            kgm, gradm, _r = step("mc", one)
        fence()
        t1 = time.perf_counter()
        for _ in range(ksteps):
            kgm, gradm, _r = step("mc", one)
        fence()
        dt = comm.max_over_ranks(time.perf_counter() - t1)
        extras["mc_shard"] = {"value": ksteps / dt, "unit": "evals/s", "ms_per_eval": 1e3 * dt / ksteps, "evals_per_step": 1,
                              "samples_per_rank": mdist.shard_samples(w.M, 0, cw)[1],
                              "collective": "one all_reduce(SUM) of %d doubles per evaluation" % (1 + w.q * w.d)}
        if rank == 0:
            r1 = G.kg_batch(w.inner_gd, w.bounds, w.discrete, one, None, w.M, best, w.kg_normals)
            sc = max(float(np.abs(r1["grad_sum"]).max()), float(np.abs(r1["kg_sum"]).max())) / w.M
            extras["mc_shard"]["max_rel_diff_vs_unsharded"] = max(float(np.abs(kgm - r1["kg_sum"] / w.M).max()),
                                                                  float(np.abs(gradm - r1["grad_sum"] / w.M).max())) / sc
        fence()
    if args.full and not args.no_batch1 and args.shard == "restarts" and multi_fallback is None:
        # one evaluation per call (what compute_grad_knowledge_gradient does): the batch-1 latency next to the batched rate
        one = my_restarts[:1]
        ksteps = max(20, args.steps)
        for _ in range(5):
            step("restarts", one)
        fence()
        t1 = time.perf_counter()
        for _ in range(ksteps):
            step("restarts", one)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t1
        extras["batch1"] = {"value": ksteps / dt, "unit": "evals/s per GPU", "ms_per_eval": 1e3 * dt / ksteps,
                            "note": "one evaluation per moe_kg_batch call, one at a time (rank 0)"}
        # and the batch of 8 the earlier rounds' headline was quoted on (comparable with BENCH_r01 / BENCH_r02)
        if R >= 8:
            eight = my_restarts[:8]
            for _ in range(2):
                step("restarts", eight)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(ksteps):
                step("restarts", eight)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t1
            extras["batch8"] = {"value": 8 * ksteps / dt, "unit": "evals/s per GPU", "ms_per_eval": 1e3 * dt / (8 * ksteps),
                                "note": "8 evaluations per moe_kg_batch call (the step of rounds 1 and 2)"}
        fence()

    if rank == 0:
        # ---- roofline of the dominant kernel (MC inner optimisation: FP64 vector-ALU bound) ----
        Rl = R if multi_fallback is None else (evals_per_step + len(gps) - 1) // len(gps)   # evaluations per launch on this device
        local_evals = Rl * args.steps                     # evaluations whose kernels this rank launched
        mc_ms = ms_mc / args.steps / (1 if multi_fallback is None else 1)   # avg MC-kernel ms per evaluation (HIP events, library stream)
        npts, f_val, f_grad = pass_flops(w)
        n_local = w.M if args.shard == "restarts" else mdist.shard_samples(w.M, 0, cw)[1]
        if multi_fallback is not None:                    # counters are summed over the devices
            S = val_passes / float(evals_per_step * args.steps * n_local)
            Gp = grad_passes / float(evals_per_step * args.steps * n_local)
        else:
            S = val_passes / float(local_evals * n_local)     # counted value passes per sample
            Gp = grad_passes / float(local_evals * n_local)   # counted value+gradient passes per sample
        flops = n_local * npts * (S * f_val + Gp * f_grad)    # per evaluation
        ach_tflops = flops / (mc_ms * 1e-3) / 1e12
        # ---- roofline of the covariance-assembly kernel (HBM write-bound) ----
        # The q-KG gradient tail no longer materialises T = K(X, x*) (kg.hip: launch_fused_tail), so the assembly kernel
        # (a3/a4: GP build, posterior queries, the d-KG tail) is measured live on an N x M shape of the size the tail used to
        # build -- N = n training rows x 80 000 columns, 640 MB at C3 -- through moe_cov_build_probe (HIP events on the
        # library's stream around `repeat` launches).
        if args.full:
            Rp = min(Rl, 8)
            probe_pts = np.random.default_rng(7).uniform(size=(Rp * n_local, w.d))
            cov_launch_ms, cov_bytes_launch = G.cov_build_probe(probe_pts, repeat=10)
            cov_bytes = cov_bytes_launch / Rp                                   # 8[nA d + nB d + nA nB]
            cov_tbs = cov_bytes_launch / (cov_launch_ms * 1e-3) / 1e12 if cov_launch_ms > 0 else 0.0
        # (which MC kernel the library launched for this shape: wave-per-sample, workgroup-per-sample, or streamed-weights -- r3)
        kinfo = G.last_kernel_info()
        mc_kernel = {0: "kg_mc_kernel", 1: "kg_mc_block_kernel", 2: "kg_mc_stream_kernel"}[kinfo["variant"]]
        if kinfo["variant"] == 0 and kinfo.get("lane"):
            mc_kernel = "kg_mc_lane_kernel"   # r5: the lane-parked form of the LDS-table kernel (csrc/kg_mc_lane.hpp)
        pmc, traffic_src = (None, "skipped (--no-traffic)" if args.full else "measured with --full")
        if args.full and world == 1 and not args.no_traffic:
            pmc, traffic_src = measure_traffic(args.config if args.derivs is None else "%s:g=%d" % (args.config, args.derivs), Rl, log)
        if pmc is None:
            pmc = committed_traffic()
            traffic_src = "profiles/hbm_traffic.json (committed rocprofv3 PMC passes of an earlier run, %d evaluations per launch; %s)" % (
                int(pmc.get("evals_per_launch", 8)), traffic_src)
        pk = pmc.get(mc_kernel, {}) if isinstance(pmc.get(mc_kernel, {}), dict) else {}
        pmc_R = int(pmc.get("evals_per_launch", 8))   # (the committed file of rounds 1-2 was taken at 8 evaluations per launch)
        traffic = pk.get("hbm_bytes_per_launch")
        exec_flop = pk.get("executed_fp64_flop_per_launch")
        launch_ms = mc_ms * Rl
        executed = None
        if exec_flop is not None and launch_ms > 0:
            ex_tflops = exec_flop * (Rl / float(pmc_R)) / (launch_ms * 1e-3) / 1e12
            executed = {"achieved": ex_tflops, "frac": ex_tflops / FP64_PEAK_TFLOPS, "flop_per_launch": exec_flop * (Rl / float(pmc_R)),
                        "wave_insts_per_launch": {k: pk[k] for k in pk if k.startswith("SQ_INSTS_VALU")},
                        "note": "EXECUTED FP64 flop (64 lanes x (2 FMA + ADD + MUL) wave-instructions, rocprofv3 PMC) / the same "
                                "HIP-event launch time: how busy the FP64 pipe is, next to the algorithmic fraction `frac`"}
        # r4: effective clock and VALU-busy fraction of the MC kernel from its own PMC passes (tools/hbm_traffic.py): GRBM_GUI_ACTIVE
        # summed over the 8 XCDs / kernel time = clock; SQ_ACTIVE_INST_VALU (quad-cycles, summed over the SIMDs) / CUs / GUI_ACTIVE
        # per XCD = the fraction of cycles a CU's vector ALUs execute an instruction (rocprofv3's own VALUBusy expression)
        in_kernel = None
        if pk.get("effective_clock_ghz") is not None:
            in_kernel = {k: pk.get(k) for k in ("effective_clock_ghz", "valu_busy", "salu_busy", "valu_insts_per_launch",
                                                 "valu_quad_cycles_per_inst", "wait_inst_frac_of_wave_cycles", "kernel_ms_under_pmc")}
            in_kernel["fp64_peak_at_effective_clock_tflops"] = 256 * 4 * 16 * 2 * pk["effective_clock_ghz"] / 1e3
            if executed and pk.get("kernel_ms_under_pmc"):
                in_kernel["executed_frac_of_peak_at_effective_clock"] = (
                    exec_flop / (pk["kernel_ms_under_pmc"] * 1e-3) / 1e12 / in_kernel["fp64_peak_at_effective_clock_tflops"])
            if pk.get("valu_insts_per_launch") and exec_flop:
                fp64_insts = sum(pk.get(k, 0.0) for k in ("SQ_INSTS_VALU_FMA_F64", "SQ_INSTS_VALU_ADD_F64", "SQ_INSTS_VALU_MUL_F64",
                                                           "SQ_INSTS_VALU_TRANS_F64"))
                in_kernel["fp64_share_of_valu_insts"] = fp64_insts / pk["valu_insts_per_launch"]
                in_kernel["fma_share_of_fp64_insts"] = pk.get("SQ_INSTS_VALU_FMA_F64", 0.0) / fp64_insts if fp64_insts else None
            in_kernel["note"] = ("PMC passes over tools/prof_kg.py (the same batched evaluation, kernel time taken from the pass itself: "
                                 "profiled runs clock lower than the timed region)")
        out = {
            "metric": ("q-KG gradient evals/s (n=1000,d=8,q=4,10k MC)" if args.config in ("C3", "C4") else
                       "%s gradient evals/s (n=%d,d=%d,q=%d,g=%d,%d MC) [secondary configuration %s]"
                       % ("d-KG" if w.g else "q-KG", w.n, w.d, w.q, w.g, w.M, args.config)),
            "value": value, "unit": "evals/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "strong" if (strong or args.shard == "mc") else "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "%s: %s value+gradient, n=%d d=%d q=%d g=%d M=%d MC, P=%d discrete pts, Matern-5/2, inner GD "
                                   "(1,6,1,3,0,1,0.1,1e-10); %s"
                                   % (args.config, "d-KG" if w.g else "q-KG", w.n, w.d, w.q, w.g, w.M, w.P,
                                      ("one step = the C4 job: %d multistart restarts, %d per GPU" % (C4_RESTARTS, R)) if strong
                                      else "%d evaluations per GPU per step" % R),
                       "shard": args.shard, "evals_per_step": evals_per_step, "evals_per_gpu_per_step": Rl},
            "rccl_ranks": comm.rccl_ranks,
            "collective_backend": comm.backend if multi_fallback is None else "none (moe_kg_batch_multi, one host thread per device)",
            "fallback": ("moe_kg_batch_multi: " + multi_fallback) if multi_fallback is not None else comm.fallback,
            "devices_used": eff_world,
            "per_rank_evals_per_s": per_rank,
            "roofline": {"bound": "fp64_valu", "achieved": ach_tflops, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": ach_tflops / FP64_PEAK_TFLOPS,
                         "executed_frac": executed["frac"] if executed else None,
                         "executed": executed,
                         "in_kernel": in_kernel,
                         "traffic": traffic * (Rl / float(pmc_R)) if traffic is not None else None,
                         "traffic_source": traffic_src,
                         "kernel": mc_kernel, "avg_launch_ms": launch_ms, "avg_ms_per_eval": mc_ms,
                         "evals_per_launch": Rl, "value_passes_per_sample": S, "grad_passes_per_sample": Gp,
                         "points_per_pass": npts, "flops_per_point_value_pass": f_val, "flops_per_point_gradient_pass": f_grad,
                         "note": "FP64 vector-ALU bound (sqrt + exp per covariance entry).  The kernel issues no MFMA: on gfx950 "
                                 "v_mfma_f64 and FP64 VALU instructions do not overlap (measured: profiles/"
                                 "r02_coissue_mfma_vs_valu.txt) and both peak at 78.6 TFLOP/s, the peak used here.  achieved = "
                                 "SURVEY 8(d) algorithmic flops -- n + u points per pass x [S f_value + G f_gradient] with the "
                                 "DEVICE-COUNTED passes S, G (bench.py: pass_flops; with derivative observations a point's 1 + g "
                                 "entries share one sqrt / exp) -- / HIP-event kernel time on the library's stream; one launch "
                                 "covers all evaluations of a step; traffic = HBM bytes per launch (PMC), tiny next to the "
                                 "compute time"},
            "kernel_ms_per_eval": {"mc": mc_ms, "cov_build": ms_cov / args.steps, "tail": ms_tail / args.steps,
                                   "state_host": ms_state / args.steps},
            "rccl_preflight_s": comm.preflight_s,
        }
        if args.full:
            out["roofline_cov_build"] = {"bound": "hbm", "achieved": cov_tbs * 1e3, "peak": HBM_PEAK_TBS * 1e3, "unit": "GB/s",
                                         "frac": cov_tbs / HBM_PEAK_TBS,
                                         # (r5: tools/prof_kg.py's probe launch has this very shape -- min(R, 8) x M columns -- whatever R)
                                         "traffic": (pmc.get("cov_build_kernel") or {}).get("hbm_bytes_per_launch"),
                                         "traffic_source": traffic_src,
                                         "kernel": "cov_build_kernel, N x M = %d x %d, measured by moe_cov_build_probe (the q-KG "
                                                   "tail itself no longer writes this matrix: it recomputes the entries where "
                                                   "they are consumed)" % (w.n, Rp * n_local),
                                         "avg_launch_ms": cov_launch_ms, "bytes_per_launch": cov_bytes_launch,
                                         "bytes_per_eval_equiv": cov_bytes}
        out.update(extras)
        if args.full and not args.no_extras:
            try:   # what the chip sustains on pure FP64 FMA chains (the clock does not hold 2.4 GHz under FP64 load)
                sus = mapi.fp64_rate(local_rank)
                out["roofline"]["sustained_fma_tflops"] = sus
                out["roofline"]["frac_of_sustained"] = ach_tflops / sus
                if executed:
                    out["roofline"]["executed_frac_of_sustained"] = executed["achieved"] / sus
            except Exception as e:  # pragma: no cover
                log("fp64_rate failed: %s" % e)
        if args.full and not args.no_extras and world == 1 and hasattr(mapi, "kxx_build_probe"):
            try:
                out["roofline_cov_build_kxx"] = mapi.kxx_build_probe(log)
            except Exception as e:  # pragma: no cover
                log("kxx_build_probe failed: %s" % e)
        # r6: scalars a driver that trims nested objects still records, and every other BASELINE configuration in one object
        if args.full:
            out["cov_build_frac"] = out["roofline_cov_build"]["frac"]
        if isinstance(out.get("roofline_cov_build_kxx"), dict):
            kx = out["roofline_cov_build_kxx"]
            fr = [v.get("frac") for v in kx.values() if isinstance(v, dict) and v.get("frac") is not None] if "frac" not in kx else [kx["frac"]]
            out["kxx_frac"] = max(fr) if fr else None
        if args.full and not args.no_extras and world == 1 and args.config in ("C3", "C4") and multi_fallback is None:
            G.close()   # (the headline GP: its workspaces go back to the pool before the other configurations build theirs)
            t_side = time.perf_counter()
            out["configs"] = side_configs(local_rank, log, c5_traffic=not args.no_traffic)
            out["configs"]["C3"] = {"evals_per_s": value, "frac": out["roofline"]["frac"], "kernel": mc_kernel}
            out["configs"]["C4"] = {"ms_per_64_restart_step": 1e3 * elapsed / args.steps,
                                    "note": "one step of this line IS the C4 job on %d GPU(s)" % world}
            out["configs"]["seconds_spent"] = time.perf_counter() - t_side
            for key, field in (("C5", "evals_per_s"), ("C5", "frac"), ("suggest", "s_per_suggestion"), ("suggest_c3", "s_per_suggestion"), ("C2", "value_grad_us"), ("C1", "mean_1pt_us")):
                if field in out["configs"].get(key, {}):
                    out["%s_%s" % (key.lower(), field)] = out["configs"][key][field]
        if args.full and not args.no_cpu_baseline and world == 1 and args.config == "C5" and args.derivs is None:
            out["cpu_baseline"] = cpu_baseline_c5(w, log)
            out["speedup_vs_cpu_one_core"] = value / out["cpu_baseline"]["value"]
        elif args.full and not args.no_cpu_baseline and world == 1 and args.derivs is None:  # reported baseline: rank 0 at N = 1 only
            out["cpu_baseline"] = cpu_baseline(w, best, args.cpu_sample_mc, log)
            out["speedup_vs_cpu_best"] = value / out["cpu_baseline"]["value"]
            if "one_core_evals_per_s" in out["cpu_baseline"]:
                out["speedup_vs_cpu_one_core"] = value / out["cpu_baseline"]["one_core_evals_per_s"]
        print(json.dumps(out), flush=True)
    comm.close()


if __name__ == "__main__":
    main()
