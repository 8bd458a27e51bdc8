// wave.hpp -- the wavefront (64 lanes) and workgroup reductions, the wavefront-local LDS synchronisation and the padded
// four-double load, one definition each.  The order of a reduction is part of what the kernels promise (bitwise equal on
// all ranks, numpy-exact sums), so each helper states which lanes hold the result, its order and what it does with NaN.
// A new kernel takes its reductions from here; a new order gets a new named helper here.  Open-coded on purpose: scans
// (__shfl_up), quadform.hip's partial butterflies (xor 16 and 32 only), lsq.hip's paired argmax, lane broadcasts -- and
// nine loops that ARE an order below, where reductions share a loop or a call changes the kernel's generated code; each
// names the helper it restates (tests/test_abi_and_host.py keeps the list).
#pragma once
#ifdef __HIPCC__
namespace beatamd {

// ---- operations: apply(m, o), m = the lane's own value, o = the other lane's; two that differ on NaN or in operand
// order are two operations
struct OpAdd {          // m + o, never contracted
    template <class T> static __device__ __forceinline__ T apply(T m, T o)
    {
#pragma clang fp contract(off)
        return m + o;
    }
};
struct OpFmax { static __device__ __forceinline__ double apply(double m, double o) { return fmax(m, o); } };  // drops a NaN
struct OpFmin { static __device__ __forceinline__ double apply(double m, double o) { return fmin(m, o); } };  // drops a NaN
struct OpMax { template <class T> static __device__ __forceinline__ T apply(T m, T o) { return max(m, o); } };  // integers
struct OpMin { template <class T> static __device__ __forceinline__ T apply(T m, T o) { return min(m, o); } };  // integers
// o > m ? o : m -- exact on unsigned long long; on doubles a NaN in o is dropped, a NaN in m stays
struct OpSelGreater { template <class T> static __device__ __forceinline__ T apply(T m, T o) { return o > m ? o : m; } };

// ---- wavefront reductions; all 64 lanes call.
// Butterfly, xor 32, 16, ..., 1: a level combines the same two values in either lane, so EVERY lane ends with the same
// bits (the operations above commute but for OpSelGreater on doubles with a NaN).
template <class Op, class T> __device__ __forceinline__ T wave_butterfly(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = Op::apply(v, __shfl_xor(v, off, 64));
    return v;
}

// Halving tree, v[l] = Op(v[l], v[l + h]) for h = 32, 16, ..., 1: LANE 0 holds the result, the other lanes hold values
// nobody may use.  Not the butterfly's order: lane 0 always has its own partial first.
template <class Op, class T> __device__ __forceinline__ T wave_tree(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = Op::apply(v, __shfl_down(v, off, 64));
    return v;
}
// wave_tree, lane 0's result in every lane
template <class Op, class T> __device__ __forceinline__ T wave_tree_bcast(T v) { return __shfl(wave_tree<Op>(v), 0, 64); }

// ---- workgroup reductions; all threads of a workgroup of whole wavefronts call.
// Butterfly per wavefront, then the wavefront values combined in wavefront order 0, 1, ... by every thread (the same bits
// in all).  sh: blockDim.x / 64 doubles, barriers before it is written and before it is read.  The sum starts from 0.0
// (-0.0 comes out as 0.0), the maximum from wavefront 0's value; fmax drops a NaN.
__device__ __forceinline__ double block_sum_waveorder(double v, double *sh)
{
    v = wave_butterfly<OpAdd>(v);
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();   // previous users of sh are done
    if ((threadIdx.x & 63) == 0) sh[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < nw; w++) s += sh[w];
    return s;
}
__device__ __forceinline__ double block_max_waveorder(double v, double *sh)
{
    v = wave_butterfly<OpFmax>(v);
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[wave] = v;
    __syncthreads();
    double s = sh[0];
    for (int w = 1; w < nw; w++) s = fmax(s, sh[w]);
    return s;
}

// Fixed-shape tree in LDS over the TB partial values of a workgroup of TB threads: red[t] = red[t] + red[t + h] for
// t < h, h = TB/2, ..., 1; every thread returns red[0].  The same order whatever the launch, and NOT the order of
// block_sum_waveorder.  red: TB doubles; a barrier before red is written, none after the last read.
template <int TB> __device__ __forceinline__ double block_sum_ldstree(double v, double *red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int h = TB / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    return red[0];
}

// ---- LDS written by one lane and read by other lanes of ITS wavefront only (no other wavefront may depend on it).
// The lanes run in lockstep: wait for the wavefront's outstanding LDS operations and keep the compiler from moving memory
// accesses across (the clobber); the wavefront barrier emits no instruction and stops the compiler's scheduler alone.
__device__ __forceinline__ void wave_lds_sync()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}
// The same promise stated to the compiler's memory model instead: release fence, wavefront barrier, acquire fence at
// wavefront scope.  The compiler places the waits itself and need not spill what the clobber above forces to memory, so
// the two generate different code: not interchangeable in a tuned kernel (hyper.hip's is this one).
__device__ __forceinline__ void wave_lds_fence_acqrel()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- v = p[k .. k + 3], zero where k + e >= M or the row is not there (!row_ok: p is not read); two double2 loads when
// the rows are 16-byte aligned (vec_ok) and all four are inside
__device__ __forceinline__ void load4_padded(const double *p, int64_t k, int64_t M, bool row_ok, int vec_ok, double (&v)[4])
{
    if (row_ok && vec_ok && k + 4 <= M) {
        const double2 a = *reinterpret_cast<const double2 *>(p + k);
        const double2 b = *reinterpret_cast<const double2 *>(p + k + 2);
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = (row_ok && k + e < M) ? p[k + e] : 0.0;
    }
}

}  // namespace beatamd
#endif
