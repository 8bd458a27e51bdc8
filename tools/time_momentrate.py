"""What the moment magnitudes, the moment-rate functions and their fuzzy density grid cost on one MI355X, against the numpy
restatement of the same arithmetic (tests/momentrate_ref.py) on the host CPU:

  legs      512 and 4096 draws of the config-3 fault (one subfault of 20 x 20 = 400 patches; uparr and uperp), deltat 0.5
  timed     magnitudes          f.magnitudes                       (k_moment_magnitude)
            moment_rates        f.moment_rates: sweep, spans, one min / max, rates   (k_moment_rate_span, k_moment_rate)
            density             the ranged density of the total curves into 500 x 500 at width 7 (k_trace_density)
  host      the restatement for ``--host-draws`` of the same draws (a Python loop over the patches, as the reference has
            one), scaled to the leg's draw count; the density's reference cost is DESIGN.md 3.9's 0.23 s per 4096-sample
            trace of draw_line_on_array -- per segment 56 us, scaled to the curves' samples (not measured again here)

    python tools/time_momentrate.py [--out profiles/momentrate_timing.json] [--reps 3]

One process, the legs alternating, wall clock around a synchronised call, the median of ``reps`` rounds after a warm-up
with min and max.  Also written: the largest |device - fixture| / bound of the rates over the cases of
tests/golden/moment_rate.npz ("rate_bound_ratio"; the bound is derived in tests/test_gpu_momentrate.py).  Nothing gates on
the timings."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "momentrate_timing.json"))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host-draws", type=int, default=32)
args = ap.parse_args()

import torch  # noqa: E402

import beat_amd  # noqa: E402
import momentrate_ref as mr  # noqa: E402
from beat_amd.synthetic import SyntheticSpec, build_problem, draw_population  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
DELTAT, GRID, WIDTH = 0.5, (500, 500), 7
REF_US_PER_SEGMENT = 0.23e6 / 4095     # draw_line_on_array, one 4096-sample trace, 500 x 500, width 7


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), n=len(v))


def rate_bound_ratio():
    from beat_amd import _lib
    worst = {}
    cases = mr.load_cases(os.path.join(ROOT, "tests", "golden", "moment_rate.npz"))
    for name, case in sorted(cases.items()):
        a = mr.case_arrays(case)
        L = _lib.FfiLayout()
        L.nparams, L.nvar = a["Q"].shape[1], len(a["comps"])
        for i in range(4):
            L.slip_off[i] = a["offs"][a["comps"][i]] if i < L.nvar else -1
        L.durations_off = a["dur_off"]
        L.velocities_off = L.nuc_strike_off = L.nuc_dip_off = L.time_off = L.h_laplacian_off = -1
        mid = ctx.ffi_model_create(L, case["ndip"], case["nstrike"], np.ones(a["nsub"]))
        offs = [a["offs"][v] for v in ("uparr", "uperp")]
        kbase, NT, dt = int(case["kbase"]), case["rates"].shape[2], float(case["deltat"])
        got = ctx.ffi_moment_rates_batch(mid, a["Q"], case["k"], a["nsub"], a["P"], dt, kbase, NT, comp_off=offs,
                                         start_times=a["starts"])
        w = 0.0
        for c in range(a["Q"].shape[0]):
            _, cover, count = mr.moment_rates(a["Q"][c], offs, case["k"], a["starts"][c], a["dur_off"], a["sub_off"],
                                              a["sub_n"], dt, kbase, NT)
            w = max(w, mr.worst_ratio(got[c] - case["rates"][c], mr.rate_bound(case["rates"][c], cover, count)))
        worst[name] = w
        ctx.ffi_model_destroy(mid)
    return worst


spec = SyntheticSpec((20,), (20,), (1.0,), T=1, N=64, D=3, S=30, slip_varnames=("uparr", "uperp"))
prob, host = build_problem(spec)
f = prob.compile(ctx)
lay, P = host["layout"], spec.P
k = np.random.default_rng(3).uniform(1.0e16, 4.0e17, P)
k_d = torch.from_numpy(k).cuda()
offs = [lay.offset(v, 0) for v in spec.slip_varnames]
dur_off = lay.offset("durations", 0)


def device_leg(C):
    pop = draw_population(spec, lay, host["lower"], host["upper"], C)
    Q = torch.from_numpy(pop).cuda()

    def density():
        res = f.moment_rates(Q, k_d, DELTAT)
        sp = res["spans"][:, -1:].contiguous()
        Y = res["rates"][:, None, :].contiguous()
        from beat_amd.summary import moment_rate_extent
        ext = np.array([moment_rate_extent(Y[:, 0].cpu().numpy(), sp[:, 0].cpu().numpy(), res["kbase"], DELTAT)])
        rg = sp.clone()
        rg[:, :, 0] -= res["kbase"]
        return Y, np.array([res["kbase"] * DELTAT]), ext, rg

    Y, tmin, ext, rg = density()
    legs = dict(magnitudes=lambda: f.magnitudes(Q, k_d), moment_rates=lambda: f.moment_rates(Q, k_d, DELTAT),
                density=lambda: ctx.trace_density_update_ranges(Y, tmin, DELTAT, ext, rg, GRID, WIDTH))
    return pop, legs, dict(draws=C, patches=P, NT=int(Y.shape[2]), segments=int((rg[:, 0, 1] - 1).clamp(min=0).sum()))


def host_leg(pop, C):
    n = min(args.host_draws, C)
    starts = f.start_times(pop[:n])
    t = time.perf_counter()
    mr.magnitudes(pop[:n], offs, k)
    t_mag = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    sp = [mr.spans(starts[c], pop[c, dur_off:dur_off + P], [0], [P], DELTAT) for c in range(n)]
    kbase = min(s[-1, 0] for s in sp)
    NT = max(s[-1].sum() for s in sp) - kbase
    for c in range(n):
        mr.moment_rates(pop[c], offs, k, starts[c], dur_off, [0], [P], DELTAT, kbase, NT)
    t_rate = (time.perf_counter() - t) * 1e3
    return dict(draws_timed=n, magnitudes_ms=t_mag * C / n, moment_rates_ms=t_rate * C / n,
                note="numpy restatement on the host, %d draws timed and scaled to %d; the sweep is not included" % (n, C))


out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "deltat": DELTAT, "grid": list(GRID), "linewidth": WIDTH,
       "what": "milliseconds per call, wall clock around a synchronised call; median of the rounds, min and max",
       "rate_bound_ratio": rate_bound_ratio(), "legs": {}}
sides = {}
for C in (512, 4096):
    sides[C] = device_leg(C)
    for fn in sides[C][1].values():        # warm-up
        fn()
ts = dict(((C, name), []) for C in sides for name in sides[C][1])
for _ in range(args.reps):
    for C in sides:
        for name, fn in sides[C][1].items():
            ts[(C, name)].append(wall(fn)[0])
for C, (pop, legs, shape) in sides.items():
    leg = dict(shape=shape, host=host_leg(pop, C))
    for name in legs:
        leg[name] = stats(ts[(C, name)])
    leg["density_reference_ms"] = shape["segments"] * REF_US_PER_SEGMENT * 1e-3
    out["legs"]["%d_draws" % C] = leg
f.release()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
