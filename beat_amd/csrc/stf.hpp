// stf.hpp -- one sample of the discretised half-sinusoid source-time function, stated once for the two kernels that
// discretise it: k_moment_rate (momentrate.hip: a patch's moment rate on the fault's time axis) and k_stf_table
// (seislib.hip: the amplitudes a Green's-function library is convolved with).  The whole rule -- rounding of the ends, the
// nt == 1 case, the fixed normalisation order -- is written at k_moment_rate; pyrocko's HalfSinusoidSTF.discretize_t as
// recalled, UNVERIFIED against pyrocko.
#pragma once
#ifdef __HIPCC__
namespace beatamd {

// a_i before normalisation: F_{i+1} - F_i, F_i = -cos((e_i - t0) w), e_i = max(t0, min(t1, tmin + (i - 0.5) deltat)),
// w = pi / duration, tmin = rint(t0 / deltat) deltat
__device__ __forceinline__ double mr_amplitude(int64_t i, double tmin, double t0, double t1, double w, double deltat)
{
#pragma clang fp contract(off)
    const double ea = fmax(t0, fmin(t1, tmin + ((double)i - 0.5) * deltat));
    const double eb = fmax(t0, fmin(t1, tmin + ((double)(i + 1) - 0.5) * deltat));
    const double fa = -cos((ea - t0) * w), fb = -cos((eb - t0) * w);
    return fb - fa;
}

}  // namespace beatamd
#endif
