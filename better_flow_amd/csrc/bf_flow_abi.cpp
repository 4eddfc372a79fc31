// bf_flow_abi.cpp -- C-ABI of the per-pixel flow field, its colour coding (EventFile::color_flow_img, event_file.h:318-350)
// and the flow frame of --flow-img / --flow-field (include/bf_accel.h, "per-pixel flow"): render_flow_field enqueues the owner
// scatter and the per-pixel pass (bf_flowimg.hip) on the context stream; bf_flow_field / bf_color_flow_img are that, a copy
// and a sync; bf_flow_frame_render runs it next to the two scale-1 projection images (render_projection_img, bf_local_abi.cpp)
// and composes the three tiles straight into a pinned, device-mapped slot in the byte layout of the files, with the ticket /
// wait / release protocol of bf_frame_* (bf_frame_abi.cpp).  Every render takes its events either from the live slice (the
// rolling optimiser's state: bf_flow_*) or from the held flow of the exhaustive search (bf_global_*, "the held flow" in
// include/bf_accel.h); nothing else differs between the two families.
#include "bf_ctx.h"

#include <vector>

namespace {

// The context's scratch for a res_x x res_y sensor (d_flow): every plane of the field, and the frame's two grey tiles.  All of
// it is written and read on the context stream, so one set per context serves every call in stream order.
struct FlowScratch {
    double *u, *v;
    uint32_t* owner;
    uint8_t *bgr, *hs, *gray[2];
};

int flow_scratch(bf_ctx* c, size_t px, FlowScratch& s) {
    HIP_TRY(c, c->d_flow.grow(c->cap_px * 27 + 64));
    uint8_t* b = c->d_flow;
    const size_t px4 = (px + 3) & ~(size_t)3;
    s.u = reinterpret_cast<double*>(b);
    s.v = s.u + px;
    s.owner = reinterpret_cast<uint32_t*>(s.v + px);
    s.bgr = reinterpret_cast<uint8_t*>(s.owner + px);
    s.hs = s.bgr + 3 * px4;
    s.gray[0] = s.hs + 2 * px4;
    s.gray[1] = s.gray[0] + px4;
    return BF_OK;
}

int flow_args(bf_ctx* c, const char* name, int32_t res_x, int32_t res_y, int32_t owner_rule) {
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "%s before bf_upload_events", name);
    if (owner_rule != BF_FLOW_LAST_UPLOADED && owner_rule != BF_FLOW_FIRST_UPLOADED)
        return fail(c, BF_ERR_ARG, "%s: unknown owner rule %d", name, owner_rule);
    if (res_x < 1 || res_y < 1 || (size_t)res_x * (size_t)res_y > c->cap_px)
        return fail(c, BF_ERR_ARG, "%s: a %d x %d sensor does not fit the context's image capacity", name, res_x, res_y);
    return BF_OK;
}

// Where a render takes its events from.  held false: the live slice, a pending bf_set_model warp applied first, (u, v) derived
// per pixel from the owner's (nx, ny).  held true: the held flow of the exhaustive search (BF_ERR_STATE without one), every
// event, (u, v) as held.
struct FlowInput {
    FlowSources e;
    const double2* uv = nullptr;   // held: the flow itself, upload order
    bool held = false;
};

int flow_input(bf_ctx* c, const char* name, bool held, FlowInput& in) {
    in.held = held;
    FlowSources& e = in.e;
    if (held) {
        GlobalHeldFlow f;
        const int rc = global_held_flow(c, name, &f);
        if (rc != BF_OK) return rc;
        e.xy = f.xy; e.p = f.p; e.perm = f.idx; e.noise = nullptr; e.nxny = f.nxny; e.n = f.n;
        in.uv = f.uv;
        return BF_OK;
    }
    const int rc = ctx_device_nxny(c, &e.nxny);   // (flushes the pending warp: the positions below are the slice's current ones)
    if (rc != BF_OK) return rc;
    const bf_ctx::EvSet& set = c->set[c->cs];
    e.xy = set.xy; e.p = set.p;
    e.perm = c->has_perm ? set.perm.get() : nullptr;
    e.noise = c->has_noise ? c->d_noise.get() : nullptr;   // (a slice with flags is never re-binned: slot == upload index)
    e.n = c->n;
    return BF_OK;
}

// The flow field of `in`, ENQUEUED on the context stream: owner plane into `owner` (res_x * res_y words), then whatever `out`
// asks for.  Arguments checked by the callers.
int render_flow_field(bf_ctx* c, const FlowInput& in, int32_t res_x, int32_t res_y, int32_t owner_rule, uint32_t* owner,
                      const FlowFieldOut& out) {
    const size_t px = (size_t)res_x * (size_t)res_y;
    HIP_TRY(c, hipMemsetAsync(owner, 0xff, px * sizeof(uint32_t), c->stream));
    {
        ProfScope ps(c, 3);
        launch_flow_owner(in.e, res_x, res_y, owner_rule == BF_FLOW_FIRST_UPLOADED ? 1 : 0, owner, c->stream);
    }
    {
        ProfScope ps(c, 3);
        if (in.held) launch_flow_field_uv(owner, in.uv, (long long)px, out, c->stream);
        else launch_flow_field(owner, in.e.nxny, (long long)px, out, c->stream);
    }
    HIP_TRY(c, hipGetLastError());
    return BF_OK;
}

}  // namespace

struct bf_flow_frame {
    int device = 0;
    int res_x = 0, res_y = 0, layouts = 0, slots = 0;
    int stride = 0;                                        // AVI row bytes
    size_t ppm_bytes = 0, avi_bytes = 0, flo_bytes = 0;    // one frame per layout
    size_t ppm_slot = 0;                                   // ppm_bytes rounded up to whole dwords (the compose kernel's stores)
    MappedArray<uint8_t> ppm, avi, flo;                    // slots x one frame
    std::vector<Event> done;                               // per slot: its render and compose have run
    // host bookkeeping, under mu
    std::mutex mu;
    long long issued = 0;
    std::vector<long long> ticket;                         // per slot: the ticket it holds, or -1 (free)
};

namespace {

int flow_frame_slot(const bf_flow_frame* f, long long t) {   // the slot holding ticket t, or -1
    if (t < 0) return -1;
    for (int s = 0; s < f->slots; ++s)
        if (f->ticket[s] == t) return s;
    return -1;
}

int flow_create_failed(bf_ctx* c, hipError_t err, const char* what) {
    return fail(c, err == hipErrorOutOfMemory ? BF_ERR_CAPACITY : BF_ERR_HIP, "bf_flow_frame_create: %s: %s", what, hipGetErrorString(err));
}

}  // namespace

// What the entry points of the two families do; `name` / `held` say which family's call it is.
namespace {

int flow_field(bf_ctx* c, const char* name, bool held, int32_t res_x, int32_t res_y, int32_t owner_rule, int32_t* owner_out,
               double* u_out, double* v_out) {
    if (!c) return BF_ERR_ARG;
    int rc = flow_args(c, name, res_x, res_y, owner_rule);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    FlowInput in;
    if ((rc = flow_input(c, name, held, in)) != BF_OK) return rc;
    const size_t px = (size_t)res_x * (size_t)res_y;
    FlowScratch s;
    if ((rc = flow_scratch(c, px, s)) != BF_OK) return rc;
    FlowFieldOut o;
    memset(&o, 0, sizeof(o));
    o.u = u_out ? s.u : nullptr;
    o.v = v_out ? s.v : nullptr;
    // (the owner plane itself holds -1 where there is no event: read as int32 it is owner_out)
    if ((rc = render_flow_field(c, in, res_x, res_y, owner_rule, s.owner, o)) != BF_OK) return rc;
    if (owner_out) HIP_TRY(c, hipMemcpyAsync(owner_out, s.owner, px * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (u_out) HIP_TRY(c, hipMemcpyAsync(u_out, s.u, px * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (v_out) HIP_TRY(c, hipMemcpyAsync(v_out, s.v, px * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BF_OK;
}

int color_flow_img(bf_ctx* c, const char* name, bool held, int32_t res_x, int32_t res_y, int32_t owner_rule, uint8_t* bgr_out,
                   uint8_t* hs_out) {
    if (!c || !bgr_out) return BF_ERR_ARG;
    int rc = flow_args(c, name, res_x, res_y, owner_rule);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    FlowInput in;
    if ((rc = flow_input(c, name, held, in)) != BF_OK) return rc;
    const size_t px = (size_t)res_x * (size_t)res_y;
    FlowScratch s;
    if ((rc = flow_scratch(c, px, s)) != BF_OK) return rc;
    FlowFieldOut o;
    memset(&o, 0, sizeof(o));
    o.bgr = s.bgr;
    o.hs = hs_out ? s.hs : nullptr;
    if ((rc = render_flow_field(c, in, res_x, res_y, owner_rule, s.owner, o)) != BF_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(bgr_out, s.bgr, px * 3, hipMemcpyDeviceToHost, c->stream));
    if (hs_out) HIP_TRY(c, hipMemcpyAsync(hs_out, s.hs, px * 2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BF_OK;
}

int flow_frame_render(bf_ctx* c, const char* name, bool held, bf_flow_frame* f, int32_t owner_rule, int64_t* ticket_out) {
    if (!c || !f || !ticket_out) return BF_ERR_ARG;
    *ticket_out = -1;
    if (c->device != f->device) return fail(c, BF_ERR_ARG, "%s: frame state on device %d, context on device %d", name, f->device, c->device);
    int rc = flow_args(c, name, f->res_x, f->res_y, owner_rule);
    if (rc != BF_OK) return rc;
    std::lock_guard<std::mutex> g(f->mu);
    int slot = -1;
    for (int s = 0; s < f->slots && slot < 0; ++s)
        if (f->ticket[s] < 0) slot = s;
    if (slot < 0) return fail(c, BF_ERR_CAPACITY, "%s: all %d frame slots are taken: release one first", name, f->slots);
    HIP_TRY(c, hipSetDevice(c->device));
    FlowInput in;
    if ((rc = flow_input(c, name, held, in)) != BF_OK) return rc;
    const size_t px = (size_t)f->res_x * (size_t)f->res_y;
    FlowScratch s;
    if ((rc = flow_scratch(c, px, s)) != BF_OK) return rc;
    const bool picture = (f->layouts & (BF_FRAME_PPM | BF_FRAME_AVI)) != 0;
    FlowFieldOut o;
    memset(&o, 0, sizeof(o));
    o.bgr = picture ? s.bgr : nullptr;
    o.flo = (f->layouts & BF_FLOW_FRAME_FLO) ? reinterpret_cast<float2*>(f->flo + (size_t)slot * f->flo_bytes) : nullptr;
    if ((rc = render_flow_field(c, in, f->res_x, f->res_y, owner_rule, s.owner, o)) != BF_OK) return rc;
    if (picture) {
        // the visualiser's other two images: projection_img(1) of the compensated events (left) and of the raw ones (right)
        // (held: of the held positions and of the same events' raw ones)
        for (int i = 0; i < 2; ++i) {
            rc = held ? render_projection_img_of(c, in.e.xy, in.e.p, nullptr, in.e.n, 1, f->res_x, f->res_y, i, s.gray[i])
                      : render_projection_img(c, 1, f->res_x, f->res_y, i, s.gray[i]);
            if (rc != BF_OK) return rc;
        }
        bf::FlowFrameCompose a;
        std::memset(&a, 0, sizeof(a));
        a.left = s.gray[0]; a.flow = s.bgr; a.right = s.gray[1];
        a.R = f->res_x; a.C = f->res_y;
        a.ppm = (f->layouts & BF_FRAME_PPM) ? f->ppm + (size_t)slot * f->ppm_slot : nullptr;
        a.avi = (f->layouts & BF_FRAME_AVI) ? f->avi + (size_t)slot * f->avi_bytes : nullptr;
        a.ppm_dwords = (long long)(f->ppm_slot / 4);
        a.avi_dwords = (long long)(f->avi_bytes / 4);
        a.stride = f->stride;
        bf::launch_flow_frame_compose(a, c->stream);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(f->done[slot], c->stream));
    f->ticket[slot] = f->issued;
    *ticket_out = f->issued++;
    return BF_OK;
}

int render_flow_frame(bf_ctx* c, bool held, int32_t res_x, int32_t res_y, int32_t owner_rule, uint8_t* ppm_out, uint8_t* avi_out, float* flo_out) {
    if (!c || (!ppm_out && !avi_out && !flo_out)) return BF_ERR_ARG;
    bf_flow_frame* f = nullptr;
    int rc = bf_flow_frame_create(c, res_x, res_y, 1, (ppm_out ? BF_FRAME_PPM : 0) | (avi_out ? BF_FRAME_AVI : 0) | (flo_out ? BF_FLOW_FRAME_FLO : 0), &f);
    if (rc != BF_OK) return rc;
    int64_t t = -1;
    const uint8_t *ppm = nullptr, *avi = nullptr;
    const float* flo = nullptr;
    if ((rc = (held ? bf_global_flow_frame_render : bf_flow_frame_render)(c, f, owner_rule, &t)) == BF_OK && (rc = bf_flow_frame_wait(c, f, t, &ppm, &avi, &flo)) == BF_OK) {
        if (ppm_out) std::memcpy(ppm_out, ppm, f->ppm_bytes);
        if (avi_out) std::memcpy(avi_out, avi, f->avi_bytes);
        if (flo_out) std::memcpy(flo_out, flo, f->flo_bytes);
    }
    (void)bf_flow_frame_destroy(f);
    return rc;
}

}  // namespace

extern "C" {

int bf_flow_field(bf_ctx* c, int32_t res_x, int32_t res_y, int32_t owner_rule, int32_t* owner_out, double* u_out, double* v_out) {
    return flow_field(c, "bf_flow_field", false, res_x, res_y, owner_rule, owner_out, u_out, v_out);
}

int bf_color_flow_img(bf_ctx* c, int32_t res_x, int32_t res_y, int32_t owner_rule, uint8_t* bgr_out, uint8_t* hs_out) {
    return color_flow_img(c, "bf_color_flow_img", false, res_x, res_y, owner_rule, bgr_out, hs_out);
}

int bf_flow_frame_create(bf_ctx* c, int32_t res_x, int32_t res_y, int32_t slots, int32_t layouts, bf_flow_frame** out) {
    if (!c || !out) return BF_ERR_ARG;
    *out = nullptr;
    if (res_x < 2 || res_y < 2 || res_x > 16384 || res_y > 16384 || slots < 1 || slots > 64 || layouts < 1 ||
        (layouts & ~(BF_FRAME_PPM | BF_FRAME_AVI | BF_FLOW_FRAME_FLO)) != 0)
        return fail(c, BF_ERR_ARG, "bf_flow_frame_create: bad sensor %d x %d, slot count %d or layouts %d", res_x, res_y, slots, layouts);
    HIP_TRY(c, hipSetDevice(c->device));
    std::unique_ptr<bf_flow_frame> f(new (std::nothrow) bf_flow_frame);   // (a failure below frees what was made)
    if (!f) return fail(c, BF_ERR_CAPACITY, "bf_flow_frame_create: out of host memory");
    f->device = c->device;
    f->res_x = res_x; f->res_y = res_y; f->layouts = layouts; f->slots = slots;
    f->stride = (3 * res_y * 3 + 3) & ~3;
    f->ppm_bytes = (size_t)res_x * (size_t)(3 * res_y) * 3;
    f->ppm_slot = (f->ppm_bytes + 3) & ~(size_t)3;
    f->avi_bytes = (size_t)f->stride * (size_t)res_x;
    f->flo_bytes = (size_t)res_x * (size_t)res_y * sizeof(float2);
    hipError_t err;
    // (pinned and mapped: the kernels store the payloads straight into them)
    if ((layouts & BF_FRAME_PPM) && (err = f->ppm.grow(f->ppm_slot * (size_t)slots)) != hipSuccess) return flow_create_failed(c, err, "PPM slots");
    if ((layouts & BF_FRAME_AVI) && (err = f->avi.grow(f->avi_bytes * (size_t)slots)) != hipSuccess) return flow_create_failed(c, err, "AVI slots");
    if ((layouts & BF_FLOW_FRAME_FLO) && (err = f->flo.grow(f->flo_bytes * (size_t)slots)) != hipSuccess) return flow_create_failed(c, err, "field slots");
    f->done.resize((size_t)slots);
    for (Event& e : f->done)
        if ((err = e.create(hipEventDisableTiming)) != hipSuccess) return flow_create_failed(c, err, "events");
    f->ticket.assign((size_t)slots, -1);
    *out = f.release();
    return BF_OK;
}

int bf_flow_frame_destroy(bf_flow_frame* f) {
    if (!f) return BF_ERR_ARG;
    (void)hipSetDevice(f->device);
    for (int s = 0; s < f->slots; ++s)
        if (f->ticket[s] >= 0) (void)hipEventSynchronize(f->done[s]);   // renders in flight write into the slots
    delete f;
    return BF_OK;
}

int bf_flow_frame_render(bf_ctx* c, bf_flow_frame* f, int32_t owner_rule, int64_t* ticket_out) {
    return flow_frame_render(c, "bf_flow_frame_render", false, f, owner_rule, ticket_out);
}

int bf_flow_frame_wait(bf_ctx* c, bf_flow_frame* f, int64_t ticket, const uint8_t** ppm, const uint8_t** avi, const float** flo) {
    if (!c || !f) return BF_ERR_ARG;
    int slot;
    hipEvent_t done;
    {
        std::lock_guard<std::mutex> g(f->mu);
        slot = flow_frame_slot(f, ticket);
        if (slot < 0) return fail(c, BF_ERR_ARG, "bf_flow_frame_wait: ticket %lld is not in flight (released, or never issued)", (long long)ticket);
        done = f->done[slot];
    }
    HIP_TRY(c, hipSetDevice(f->device));
    HIP_TRY(c, hipEventSynchronize(done));
    if (ppm) *ppm = (f->layouts & BF_FRAME_PPM) ? f->ppm + (size_t)slot * f->ppm_slot : nullptr;
    if (avi) *avi = (f->layouts & BF_FRAME_AVI) ? f->avi + (size_t)slot * f->avi_bytes : nullptr;
    if (flo) *flo = (f->layouts & BF_FLOW_FRAME_FLO) ? reinterpret_cast<const float*>(f->flo + (size_t)slot * f->flo_bytes) : nullptr;
    return BF_OK;
}

int bf_flow_frame_release(bf_flow_frame* f, int64_t ticket) {
    if (!f) return BF_ERR_ARG;
    std::lock_guard<std::mutex> g(f->mu);
    const int slot = flow_frame_slot(f, ticket);
    if (slot < 0) return BF_ERR_ARG;
    (void)hipSetDevice(f->device);
    (void)hipEventSynchronize(f->done[slot]);   // (released unwaited: the kernels must not write into a slot given out again)
    f->ticket[slot] = -1;
    return BF_OK;
}

int bf_render_flow_frame(bf_ctx* c, int32_t res_x, int32_t res_y, int32_t owner_rule, uint8_t* ppm_out, uint8_t* avi_out, float* flo_out) {
    return render_flow_frame(c, false, res_x, res_y, owner_rule, ppm_out, avi_out, flo_out);
}

// ---- the same from the held flow of the exhaustive search (include/bf_accel.h, "the held flow") ----

int bf_global_flow_field(bf_ctx* c, int32_t res_x, int32_t res_y, int32_t owner_rule, int32_t* owner_out, double* u_out, double* v_out) {
    return flow_field(c, "bf_global_flow_field", true, res_x, res_y, owner_rule, owner_out, u_out, v_out);
}

int bf_global_color_flow_img(bf_ctx* c, int32_t res_x, int32_t res_y, int32_t owner_rule, uint8_t* bgr_out, uint8_t* hs_out) {
    return color_flow_img(c, "bf_global_color_flow_img", true, res_x, res_y, owner_rule, bgr_out, hs_out);
}

int bf_global_flow_frame_render(bf_ctx* c, bf_flow_frame* f, int32_t owner_rule, int64_t* ticket_out) {
    return flow_frame_render(c, "bf_global_flow_frame_render", true, f, owner_rule, ticket_out);
}

int bf_global_render_flow_frame(bf_ctx* c, int32_t res_x, int32_t res_y, int32_t owner_rule, uint8_t* ppm_out, uint8_t* avi_out,
                                float* flo_out) {
    return render_flow_frame(c, true, res_x, res_y, owner_rule, ppm_out, avi_out, flo_out);
}

}  // extern "C"
