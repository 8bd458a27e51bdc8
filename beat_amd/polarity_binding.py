"""
The Python binding of the polarity entries of ``libbeat_amd.so`` (``beatamd_ffi_model_add_polarity``, ``beatamd_mt6_batch``,
``beatamd_polarity_amplitudes_batch``, ``beatamd_w_to_beta_batch``; csrc/polarity.hip) as functions of a ``Context``
(``ctx``, beat_amd.engine).  tests/test_polarity_marshal_host.py pins what every entry receives.
"""
import numpy as np

from . import _lib
from ._lib import check, ptr
from ._marshal import as_input, checked


def check_polarity_source(kind, param_off, param_fixed, nparams=None, tables=None):
    """the argument rules of the polarity entries that need no device, checked ahead of the call (the library checks
    them again): a known source kind; six offsets in [-1, nparams) and six fixed values; for ``mtqt`` the two tables
    (u strictly increasing).  -> (kind, off int64 (6,), fix float64 (6,), ntab, utab, btab)"""
    kinds = {"mtqt": _lib.POL_MTQT, "mt": _lib.POL_MT, "dc": _lib.POL_DC}
    if kind not in kinds:
        raise ValueError("unknown polarity source kind %r (one of %s)" % (kind, ", ".join(sorted(kinds))))
    off = np.ascontiguousarray(param_off, dtype=np.int64).ravel()
    fix = np.ascontiguousarray(param_fixed, dtype=np.float64).ravel()
    if off.size != 6 or fix.size != 6:
        raise ValueError("polarity source tables hold six slots, got %d offsets and %d values" % (off.size, fix.size))
    if np.any(off < -1) or (nparams is not None and np.any(off >= nparams)):
        raise ValueError("polarity source offsets %s outside q of %s parameters" % (off.tolist(), nparams))
    utab = btab = None
    if kinds[kind] == _lib.POL_MTQT:
        if tables is None:
            from .sources import BETA_MAPPING, U_MAPPING
            tables = (U_MAPPING, BETA_MAPPING)
        utab = np.ascontiguousarray(tables[0], dtype=np.float64)
        btab = np.ascontiguousarray(tables[1], dtype=np.float64)
        if utab.ndim != 1 or utab.shape != btab.shape or utab.size < 2:
            raise ValueError("the w -> beta tables must be two vectors of one length >= 2")
        if not np.all(np.diff(utab) > 0):
            raise ValueError("the u table is not strictly increasing: numpy.interp is undefined on it")
    return kinds[kind], off, fix, (0 if utab is None else int(utab.size)), utab, btab


def ffi_model_add_polarity(ctx, model_id, kind, param_off, param_fixed, n_t, rw, obs, gamma, hp_off, hp_fixed,
                           tables=None):
    """the polarity composite of a model (``beatamd_ffi_model_add_polarity``): source ``kind`` ("mtqt", "mt",
    "dc") with its (6,) offset / fixed-value tables, per map its station count, rw (6, sum n_t), obs (sum n_t,),
    gamma, and per map the offset of its sigma in q (-1: hp_fixed)"""
    k, off, fix, ntab, utab, btab = check_polarity_source(kind, param_off, param_fixed, tables=tables)
    nt = np.ascontiguousarray(n_t, dtype=np.int64).ravel()
    rw = np.ascontiguousarray(rw, dtype=np.float64)
    ob = np.ascontiguousarray(obs, dtype=np.float64).ravel()
    ho = np.ascontiguousarray(hp_off, dtype=np.int64).ravel()
    hf = np.ascontiguousarray(hp_fixed, dtype=np.float64).ravel()
    NT = int(nt.sum())
    if rw.shape != (6, NT) or ob.shape != (NT,) or ho.shape != nt.shape or hf.shape != nt.shape:
        raise ValueError("add_polarity: %d maps of %d stations need rw (6, %d), obs (%d,) and %d hyper slots; got %s, %s, "
                         "%d" % (nt.size, NT, NT, NT, nt.size, rw.shape, ob.shape, ho.size))
    check(ctx._lib.beatamd_ffi_model_add_polarity(ctx._h, model_id, k, ptr(off), ptr(fix), int(nt.size), ptr(nt), ptr(rw),
                                                   ptr(ob), float(gamma), ptr(ho), ptr(hf), ntab, ptr(utab), ptr(btab)))


def mt6_batch(ctx, Q, kind, param_off, param_fixed, tables=None, out=None):
    """Q (C, nparams) -> (C, 6): the normalised (mnn, mee, mdd, mne, mnd, med) of every row, by the kernel the model
    launches.  numpy in -> numpy out, torch-cuda in -> tensor"""
    Q, Cn, out = ctx._q_out(Q, out, (6,))
    k, off, fix, ntab, utab, btab = check_polarity_source(kind, param_off, param_fixed, int(Q.shape[1]), tables)
    check(ctx._lib.beatamd_mt6_batch(ctx._h, k, Cn, int(Q.shape[1]), ptr(Q), ptr(off), ptr(fix), ntab, ptr(utab),
                                      ptr(btab), ptr(out)))
    return out


def polarity_amplitudes_batch(ctx, Q, kind, param_off, param_fixed, rw, tables=None, out=None):
    """Q (C, nparams) -> (C, NT): ``heart.pol_synthetics`` of every row against the propagation coefficients rw
    (6, NT) (host array)"""
    rw = np.ascontiguousarray(rw, dtype=np.float64)
    if rw.ndim != 2 or rw.shape[0] != 6 or rw.shape[1] < 1:
        raise ValueError("polarity_amplitudes_batch: rw must be (6, n_stations), got %s" % (rw.shape,))
    Q, Cn, out = ctx._q_out(Q, out, (int(rw.shape[1]),))
    k, off, fix, ntab, utab, btab = check_polarity_source(kind, param_off, param_fixed, int(Q.shape[1]), tables)
    check(ctx._lib.beatamd_polarity_amplitudes_batch(ctx._h, k, Cn, int(Q.shape[1]), ptr(Q), ptr(off), ptr(fix), ntab,
                                                      ptr(utab), ptr(btab), int(rw.shape[1]), ptr(rw), ptr(out)))
    return out


def w_to_beta_batch(ctx, w, tables=None, out=None):
    """w (n,) -> beta (n,): ``sources.w_to_beta`` by the device function of the polarity kernel, bit for bit
    ``numpy.interp`` on the tables (default: U_MAPPING / BETA_MAPPING)"""
    ctx._adopt_stream(w)
    w = as_input(w)
    _, _, _, ntab, utab, btab = check_polarity_source("mtqt", -np.ones(6), np.zeros(6), tables=tables)
    out = checked(out, w, tuple(w.shape), np.float64, "out", of="w")
    n = int(np.prod(tuple(w.shape)))
    check(ctx._lib.beatamd_w_to_beta_batch(ctx._h, n, ptr(w), ntab, ptr(utab), ptr(btab), ptr(out)))
    return out
