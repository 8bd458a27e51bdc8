// ctx.cpp -- context lifetime, staging, timing, error reporting.
#include "ctx.hpp"

#include <cstdlib>

namespace beatamd {

static thread_local char g_err[1024] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int DevBuf::reserve(size_t bytes)
{
    if (bytes <= cap) return BEATAMD_OK;
    // grow geometrically so that a sampler with slowly varying batch sizes settles
    size_t want = bytes + bytes / 4;
    if (p) {
        // kernels of earlier calls may still read the old buffer (any stream): drain first
        BA_HIP(hipDeviceSynchronize());
        BA_HIP(hipFree(p));
        p = nullptr;
        cap = 0;
    }
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        e = hipMalloc(&p, bytes);
        want = bytes;
    }
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        p = nullptr;
        return BEATAMD_ENOMEM;
    }
    cap = want;
    return BEATAMD_OK;
}

void DevBuf::release()
{
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}

bool is_device_ptr(const void *p)
{
    if (!p) return false;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // unregistered host memory
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

int dev_copy_sync(beatamd_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    BA_CHECK(e == hipSuccess, BEATAMD_EHIP, "hipMemcpy(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    return BEATAMD_OK;
}

int Staging::in_bytes(const void *p, size_t bytes, const void **dev)
{
    BA_CHECK(nin < SL_NIN, BEATAMD_EINVAL, "internal: more than %d staged inputs in one call", SL_NIN);
    const int slot = SL_IN0 + nin++;
    *dev = p;
    if (bytes == 0 || p == nullptr || is_device_ptr(p)) return BEATAMD_OK;
    void *d = nullptr;
    BA_TRY(ctx->get_scratch(slot, bytes, &d));
    BA_HIP(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, ctx->stream));
    *dev = d;
    return BEATAMD_OK;
}

int Staging::out_bytes(void *p, size_t bytes, void **dev, bool preload)
{
    BA_CHECK(nout < SL_NOUT, BEATAMD_EINVAL, "internal: more than %d staged outputs in one call", SL_NOUT);
    const int slot = SL_OUT0 + nout++;
    *dev = p;
    if (bytes == 0 || p == nullptr || is_device_ptr(p)) return BEATAMD_OK;
    void *d = nullptr;
    BA_TRY(ctx->get_scratch(slot, bytes, &d));
    if (preload) BA_HIP(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, ctx->stream));
    back[nback++] = {p, d, bytes};
    *dev = d;
    return BEATAMD_OK;
}

int Staging::finish()
{
    for (int i = 0; i < nback; i++)
        BA_HIP(hipMemcpyAsync(back[i].host, back[i].dev, back[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
    return nback ? ctx->check_status() : BEATAMD_OK;   // (synchronises)
}

int64_t FfiModel::nllk() const
{
    int64_t n = 1;  // like
    for (auto &w : wavemaps) n += w.T;
    if (has_geo) n += (int64_t)geo.sizes.size();
    if (has_pol) n += pol.NT;
    if (lap >= 0) n += 1;
    return n;
}

}  // namespace beatamd

using namespace beatamd;

int beatamd_ctx::get_scratch(int slot, size_t bytes, void **out)
{
    if ((size_t)slot >= scratch_bufs.size()) scratch_bufs.resize(slot + 1);
    BA_TRY(scratch_bufs[slot].reserve(bytes));
    *out = scratch_bufs[slot].p;
    return BEATAMD_OK;
}

hipEvent_t beatamd_ctx::get_event()
{
    if (!event_pool.empty()) {
        hipEvent_t e = event_pool.back();
        event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

void beatamd_ctx::time_begin(const char *name)
{
    if (!timing) return;
    KTimer &t = timers[name];
    hipEvent_t a = get_event(), b = get_event();
    (void)hipEventRecord(a, stream);
    t.pending.emplace_back(a, b);
}

void beatamd_ctx::time_end(const char *name)
{
    if (!timing) return;
    KTimer &t = timers[name];
    if (!t.pending.empty()) (void)hipEventRecord(t.pending.back().second, stream);
}

int beatamd_ctx::check_status()
{
    BA_HIP(hipStreamSynchronize(stream));
    int st = 0;
    BA_HIP(hipMemcpy(&st, d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (st) {
        BA_HIP(hipMemset(d_status, 0, sizeof(int)));
        if (st & ST_INDEX_OOB) {
            set_error("index out of bounds of the GF library "
                      "(duration/starttime outside the library grid)");
            return BEATAMD_EINDEX;
        }
        if (st & ST_BAD_HYPO) {
            set_error("nucleation index outside the patch grid");
            return BEATAMD_EINVAL;
        }
        if (st & ST_BAD_COV) {
            // smc.py:167-186: the text of the reference's ValueError
            set_error("Sample covariances contains Inf or NaN! Please try reducing the upper and lower bounds "
                      "of hyper parameters!");
            return BEATAMD_EBADCOV;
        }
        if (st & ST_NOT_PSD) {
            set_error("Matrix is not positive definite");   // numpy.linalg.LinAlgError's text
            return BEATAMD_ENOTPSD;
        }
        if (st & ST_LINE_NONFINITE) {
            set_error("trace_density: a sample or an extent that is not finite (or xmax <= xmin)");
            return BEATAMD_EINVAL;
        }
        if (st & ST_LINE_OOB) {
            // plotting/common.py:733-739 check_line_in_grid: the reference's TypeError
            set_error("Line endpoint outside of given grid (an index above the last cell, or below -32768)");
            return BEATAMD_EOUTSIDE;
        }
        if (st & ST_SPAN_BAD) {
            set_error("moment rate: an onset or duration that is not finite, a negative duration, or a time index beyond 2^40");
            return BEATAMD_EINVAL;
        }
        if (st & ST_SPAN_OOB) {
            set_error("moment rate: a draw's time span does not lie within the index grid [kbase, kbase + NT): its rows are NaN");
            return BEATAMD_EINVAL;
        }
        if (st & ST_BAD_SCALE) {
            set_error("PoissonProposal: a step width outside (0, 500] (or NaN): the draws of that parameter are NaN");
            return BEATAMD_EINVAL;
        }
    }
    return BEATAMD_OK;
}

namespace beatamd {

void GfKnobs::read_env()
{
    auto rd = [](const char *name) { const char *e = getenv(name); return e ? atoi(e) : KNOB_UNSET; };
#define X(member, env) member = rd(env);
    BEATAMD_GF_KNOBS(X)
#undef X
}

const GfKnobs &gf_knobs(beatamd_ctx *ctx)
{
    if (ctx->knobs_live) ctx->knobs.read_env();
    return ctx->knobs;
}

}  // namespace beatamd

extern "C" {

const char *beatamd_last_error(void) { return g_err; }

int beatamd_version(void) { return BEATAMD_VERSION; }

int beatamd_ctx_create(int device, beatamd_ctx **out)
{
    BA_CHECK(out != nullptr, BEATAMD_EINVAL, "ctx_create: out is NULL");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        set_error("no HIP device available (%s)", hipGetErrorString(e));
        return BEATAMD_EHIP;
    }
    BA_CHECK(device >= 0 && device < ndev, BEATAMD_EINVAL, "device %d out of range [0,%d)", device,
             ndev);
    BA_HIP(hipSetDevice(device));
    beatamd_ctx *c = new beatamd_ctx();
    c->device = device;
    BA_HIP(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    BA_HIP(hipMalloc((void **)&c->d_status, sizeof(int)));
    BA_HIP(hipMemset(c->d_status, 0, sizeof(int)));
    hipDeviceProp_t prop;
    BA_HIP(hipGetDeviceProperties(&prop, device));
    c->num_cu = prop.multiProcessorCount;
    c->scratch_bufs.resize(SL_COUNT);
    c->knobs.read_env();
    {
        const char *live = getenv("BEATAMD_KNOBS_LIVE");
        c->knobs_live = live && atoi(live) != 0;
    }
    *out = c;
    return BEATAMD_OK;
}

int beatamd_ctx_reload_knobs(beatamd_ctx *c)
{
    BA_CHECK(c != nullptr, BEATAMD_EINVAL, "ctx_reload_knobs: NULL context");
    c->knobs.read_env();
    return BEATAMD_OK;
}

int beatamd_ctx_destroy(beatamd_ctx *c)
{
    if (!c) return BEATAMD_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    // the objects free their device arrays (before the stream and the status word go)
    c->models.clear();
    c->hypers.clear();
    c->wsets.clear();
    c->laps.clear();
    c->geoens.clear();
    c->geolibs.clear();
    c->seislibs.clear();
    c->twiddles.clear();
    for (auto &s : c->scratch_bufs) s.release();
    for (auto &kv : c->timers)
        for (auto &pr : kv.second.pending) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    if (c->d_status) (void)hipFree(c->d_status);
    if (c->h_umax) (void)hipHostFree(c->h_umax);
    if (c->umax_event) (void)hipEventDestroy(c->umax_event);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return BEATAMD_OK;
}

int beatamd_ctx_set_stream(beatamd_ctx *c, void *s)
{
    BA_CHECK(c, BEATAMD_EINVAL, "ctx is NULL");
    BA_HIP(hipSetDevice(c->device));
    c->stream = (hipStream_t)s;  // NULL = the HIP null stream
    return BEATAMD_OK;
}

int beatamd_ctx_use_own_stream(beatamd_ctx *c)
{
    BA_CHECK(c, BEATAMD_EINVAL, "ctx is NULL");
    c->stream = c->own_stream;
    return BEATAMD_OK;
}

int beatamd_ctx_set_step_counter(beatamd_ctx *c, uint32_t *device_counter)
{
    BA_CHECK(c != nullptr, BEATAMD_EINVAL, "ctx is NULL");
    BA_CHECK(device_counter == nullptr || is_device_ptr(device_counter), BEATAMD_EINVAL,
             "ctx_set_step_counter: the counter must live in device memory");
    c->step_dev = device_counter;
    return BEATAMD_OK;
}

int beatamd_ctx_synchronize(beatamd_ctx *c)
{
    BA_CHECK(c, BEATAMD_EINVAL, "ctx is NULL");
    BA_HIP(hipSetDevice(c->device));
    return c->check_status();
}

int beatamd_ctx_enable_timing(beatamd_ctx *c, int on)
{
    BA_CHECK(c, BEATAMD_EINVAL, "ctx is NULL");
    c->timing = on != 0;
    return BEATAMD_OK;
}

static int drain_timer(beatamd_ctx *c, KTimer &t)
{
    for (auto &pr : t.pending) {
        BA_HIP(hipEventSynchronize(pr.second));
        float ms = 0.f;
        BA_HIP(hipEventElapsedTime(&ms, pr.first, pr.second));
        t.total_ms += ms;
        t.n += 1;
        c->event_pool.push_back(pr.first);
        c->event_pool.push_back(pr.second);
    }
    t.pending.clear();
    return BEATAMD_OK;
}

int beatamd_ctx_kernel_time(beatamd_ctx *c, const char *kernel, double *total_ms, int64_t *launches)
{
    BA_CHECK(c && kernel, BEATAMD_EINVAL, "bad argument");
    auto it = c->timers.find(kernel);
    if (it == c->timers.end()) {
        if (total_ms) *total_ms = 0;
        if (launches) *launches = 0;
        return BEATAMD_OK;
    }
    BA_TRY(drain_timer(c, it->second));
    if (total_ms) *total_ms = it->second.total_ms;
    if (launches) *launches = it->second.n;
    return BEATAMD_OK;
}

int beatamd_ctx_reset_timing(beatamd_ctx *c)
{
    BA_CHECK(c, BEATAMD_EINVAL, "ctx is NULL");
    for (auto &kv : c->timers) {
        BA_TRY(drain_timer(c, kv.second));
        kv.second.total_ms = 0;
        kv.second.n = 0;
    }
    return BEATAMD_OK;
}

}  // extern "C"
