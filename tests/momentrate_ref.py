"""
numpy restatement of csrc/momentrate.hip, operation by operation (test infrastructure; float64 throughout, numpy does not
contract a * b + c).  The reference lines it follows:

  beat/ffi/fault.py:343-359   get_total_slip: slips = zeros; slips += var ** 2 per component; sqrt
  beat/ffi/fault.py:284-341   get_subfault_patch_moments / get_moment / get_magnitude
  beat/ffi/fault.py:410-443   get_subfault_moment_rate_function (time axis :414-420, accumulation :436-441)
  beat/ffi/fault.py:445-474   get_moment_rate_function (the total, :460-472)
  pyrocko HalfSinusoidSTF.discretize_t (exponent 1), moment_to_magnitude: as recalled, UNVERIFIED against pyrocko

Where the device fixes an order that numpy's own reductions do not have (num.sum is pairwise), the order is restated
here: ``sum_in_patch_order`` and ``fold64``.  ``cos`` / ``log10`` are numpy's: the device's differ by a few ulp, which is
what the tolerance of the tests covers.
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)   # 2^-52


def total_slip(q, offs, P):
    """fault.py:355-359 for one draw: sqrt(((0 + s0^2) + s1^2) ...) over the variables at the offsets ``offs``"""
    s2 = np.zeros(P)
    for o in offs:
        v = q[o:o + P]
        s2 = s2 + v * v
    return np.sqrt(s2)


def patch_moments(q, offs, k):
    """fault.py:303-313: k_p * slip_p, exactly 0 for a patch without slip"""
    slip = total_slip(q, offs, k.size)
    return np.where(slip != 0.0, k * slip, 0.0)


def sum_in_patch_order(terms):
    """the device's order: one after the other from 0.0 (the reference's num.array(moments).sum() is pairwise)"""
    m0 = np.float64(0.0)
    for t in terms:
        m0 = m0 + t
    return m0


def moment_to_magnitude(m0):
    """pyrocko's formula as recalled (UNVERIFIED); fault.py:338-341: a zero moment is returned as it is"""
    return np.float64(0.0) if m0 == 0.0 else np.log10(m0 * 1.0e7) / 1.5 - 10.7


def magnitudes(Q, offs, k):
    M0 = np.array([sum_in_patch_order(patch_moments(q, offs, k)) for q in Q])
    return M0, np.array([moment_to_magnitude(m) for m in M0])


def spans(starts, durations, sub_off, sub_n, deltat):
    """fault.py:414-417 and :461-465 for one draw -> (nsub + 1, 2) int64 = (first index, count), the total last"""
    dmax = durations.max()
    out = np.zeros((len(sub_off) + 1, 2), dtype=np.int64)
    for s, (o, n) in enumerate(zip(sub_off, sub_n)):
        st = starts[o:o + n]
        first = int(np.floor(st.min() / deltat))
        out[s] = first, int(np.ceil((st.max() + dmax) / deltat)) + 1 - first
    first = out[:-1, 0].min()
    out[-1] = first, (out[:-1, 0] + out[:-1, 1]).max() - first
    return out


def fold64(a):
    """the FIXED normalisation order of k_moment_rate: lane l adds a_l, a_{l+64}, ... one after the other from 0.0, the 64
    lane sums are folded 32 / 16 / 8 / 4 / 2 / 1"""
    pad = np.zeros(((a.size + 63) // 64) * 64)
    pad[:a.size] = a
    part = np.zeros(64)
    for row in pad.reshape(-1, 64):
        part = part + row
    n = 32
    while n >= 1:
        part = part[:n] + part[n:2 * n]
        n //= 2
    return part[0]


def half_sinusoid(t0, duration, deltat, cos=np.cos, total=fold64):
    """-> (k0, amplitudes [nt]).  ``cos`` / ``total``: replaceable, for the test that shows what the bound catches and for
    the reference's own num.sum"""
    t1 = t0 + duration
    r0, r1 = np.rint(t0 / deltat), np.rint(t1 / deltat)
    k0, nt = int(r0), int(r1) - int(r0) + 1
    if nt == 1:
        return k0, np.ones(1)
    tmin = r0 * deltat
    edges = np.maximum(t0, np.minimum(t1, tmin + (np.arange(nt + 1) - 0.5) * deltat))
    F = -cos((edges - t0) * (np.pi / duration))
    a = F[1:] - F[:-1]
    return k0, a / total(a)


def moment_rates(q, offs, k, starts, dur_off, sub_off, sub_n, deltat, kbase, NT, cos=np.cos, total=fold64):
    """one draw -> rates (nsub + 1, NT) on the index grid [kbase, kbase + NT), cover (nsub + 1, NT) = sum of the moments
    of the patches whose support holds the sample, count (nsub + 1, NT) = how many they are (both for the tolerance)"""
    P = k.size
    m = patch_moments(q, offs, k)
    nsub = len(sub_off)
    rates, cover, count = np.zeros((nsub + 1, NT)), np.zeros((nsub + 1, NT)), np.zeros((nsub + 1, NT), dtype=np.int64)
    for s, (o, n) in enumerate(zip(sub_off, sub_n)):
        for p in range(o, o + n):
            k0, a = half_sinusoid(starts[p], q[dur_off + p], deltat, cos, total)
            sl = slice(k0 - kbase, k0 - kbase + a.size)
            rates[s, sl] = rates[s, sl] + a * m[p]
            cover[s, sl] += m[p]
            count[s, sl] += 1
    for s in range(nsub):                      # fault.py:466-472: zeros, += every subfault in order
        rates[nsub] = rates[nsub] + rates[s]
    cover[nsub], count[nsub] = cover[:nsub].sum(0), count[:nsub].sum(0)
    return rates, cover, count


def rate_bound(ref, cover, count):
    """the issue's element-wise bound: 16 eps sum_{p covering j} m_p + 4 eps n_j |ref_j|"""
    return 16.0 * EPS * cover + 4.0 * EPS * count * np.abs(ref)


def worst_ratio(diff, bound):
    """largest |diff| / bound over the elements with a positive bound (0.0 where there is none)"""
    ok = bound > 0
    return float((np.abs(diff)[ok] / bound[ok]).max()) if ok.any() else 0.0


# ---- the fixture tests/golden/moment_rate.npz (tools/gen_golden_momentrate.py) as the tests use it
def load_cases(path):
    z = np.load(path)
    cases = {}
    for name in z["cases"]:
        pre = "%s_" % name
        cases[str(name)] = dict((key[len(pre):], z[key]) for key in z.files if key.startswith(pre))
    return cases


def case_arrays(case):
    """the parameter vectors of a case: q = [slip variables ..., durations], P entries each.  -> dict(Q (C, nparams),
    offs (name -> offset), dur_off, sub_off, sub_n, starts (C, P) = onsets + the subfault's time, P, nsub)"""
    comps = [str(c) for c in case["comps"]]
    P = int(case["k"].size)
    sub_n = [int(d) * int(s) for d, s in zip(case["ndip"], case["nstrike"])]
    sub_off = [int(v) for v in np.cumsum([0] + sub_n[:-1])]
    Q = np.ascontiguousarray(np.concatenate([case[c] for c in comps] + [case["durations"]], axis=1))
    offs = dict((c, i * P) for i, c in enumerate(comps))
    starts = case["onsets"].copy()
    for s, (o, n) in enumerate(zip(sub_off, sub_n)):
        starts[:, o:o + n] = case["onsets"][:, o:o + n] + case["time"][:, s:s + 1]
    return dict(Q=Q, offs=offs, comps=comps, dur_off=len(comps) * P, sub_off=sub_off, sub_n=sub_n, starts=starts, P=P,
                nsub=len(sub_n))
