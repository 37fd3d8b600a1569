// car_render.hip — the one-call forward of the C ABI (include/car_hip.h: car_plan_*, car_project_maps, car_render_forward).
//
// Host-side C++: it carves the caller's plan / workspace buffers, has every layer packed into the operand order of the kernels that consume
// it (car_pack.hip, the kernels' own packers), merges the projected maps (car_lattice.hip) and issues the launch sequence of the default configuration
// (CrossAttentionRenderer(model="midas_vit", n_view=2), reference models.py:190-626) from plain pointers.  This IS the product
// path: cross_attention_renderer_amd/engine.py calls it for that configuration (its own stage-by-stage sequence covers the
// constructor variants and serves as the A/B partner in tests/test_hip_parity.py).
#include "car_common.h"
#include "car_geom.h"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

#include "car_fused_layout.h"
#include "car_chain_layout.h"

constexpr size_t kRound = 64;                                        // every piece of this unit's buffers is a whole number of 64 floats

// ---- plan layout ---------------------------------------------------------------------------------------------------
struct Plan {
    // offsets in floats.  chain[slot]: car_chain_pack tiles of the per-ray chains' layers (car_chain_layout.h); chain_scale: their powers
    // of two; mid_bias / tail_bias: their biases in consumption order
    size_t steps, blob, fbias, wpt, r2qw, r2qb, proj[CAR_MAX_LEVELS], proj16[CAR_MAX_LEVELS], chain[kChainLayers], chain_scale, mid_bias, tail_bias, total;
};
// car_linear_x3 wants rows of whole float4s and a K worth its 32-wide chunks; narrower levels stay on car_linear
inline bool level_on_f16_pipe(int c) { return c % 4 == 0 && c >= 32; }
Plan plan_layout(const car_dims& d) {
    Plan p;
    Carver c(nullptr, kRound);
    auto take = [&](size_t n) { return c.at<float>(n); };
    p.steps = take((size_t)d.P);
    p.blob = take(car_fused_blob_floats());
    p.fbias = take(car_fused_bias_floats());
    p.wpt = take((size_t)kC * 4);
    p.r2qw = take(car_round2q_packed_floats());
    p.r2qb = take(car_round2q_bias_floats());
    for (int l = 0; l < CAR_MAX_LEVELS; ++l) p.proj[l] = l < d.n_levels ? take(car_linear_packed_floats(d.level_c[l], kC)) : 0;
    // the same slices for the split-fp16 kernel (car_linear_x3), which car_project_maps takes for the levels it serves
    for (int l = 0; l < CAR_MAX_LEVELS; ++l) p.proj16[l] = (l < d.n_levels && level_on_f16_pipe(d.level_c[l])) ? take(car_linear_x3_packed_floats(d.level_c[l], kC)) : 0;
    for (int slot : kPlanOrder) p.chain[slot] = take(chain_floats(slot));
    p.chain_scale = take(kScaleFloats);
    p.mid_bias = take(kMidBiasFloats);
    p.tail_bias = take(kTailBiasFloats);
    p.total = c.bytes() / sizeof(float);
    return p;
}

int check_dims(const car_dims* d, const char* who) {
    CAR_REQUIRE(d, "%s: null dims", who);
    CAR_REQUIRE(d->b > 0 && d->R > 0 && d->P > 1 && d->H > 1 && d->W > 1, "%s: bad sizes", who);
    CAR_REQUIRE(d->V == 2 && d->n_levels == 3, "%s: the one-call forward covers n_view = 2 and three pyramid levels (got %d, %d); "
                "other configurations run through the stage entries", who, d->V, d->n_levels);
    int csum = 0;
    for (int l = 0; l < d->n_levels; ++l) {
        CAR_REQUIRE(d->level_h[l] > 0 && d->level_w[l] > 0 && d->level_c[l] > 0, "%s: bad level %d", who, l);
        csum += d->level_c[l];
    }
    CAR_REQUIRE(csum == kC, "%s: the levels' channels must add up to %d (got %d)", who, kC, csum);
    CAR_REQUIRE(2 * d->P <= 128 * 3, "%s: too many samples per ray", who);
    CAR_REQUIRE(car_lattice_of(*d).ok, "%s: every pyramid level must be an integer factor coarser than the widest one, the same factor in both "
                "directions (the fused kernel gathers them from their common lattice); other pyramids run through the stage entries", who);
    return CAR_OK;
}

// ---- workspace layout ----------------------------------------------------------------------------------------------
struct Span { size_t off, cnt; };                                   // one buffer: offset and element count, in floats
struct Work {
    Span rays, phi_x, e, g, logit, logit2, pt, pixel_val, coords, at_wt, at_wt2, amax, depth, ebar, z1, uh, valid, part;
    size_t total;
};
// the buffers car_workspace_find hands out (include/car_hip.h lists them)
const struct { const char* name; Span Work::*buf; } kFindable[] = {
    {"rays", &Work::rays}, {"e", &Work::e}, {"g", &Work::g}, {"logit", &Work::logit}, {"logit2", &Work::logit2}, {"pt", &Work::pt},
    {"at_wt2", &Work::at_wt2}, {"ebar", &Work::ebar}, {"z1", &Work::z1}, {"uh", &Work::uh}, {"part", &Work::part}, {"phi_x", &Work::phi_x}};
// step groups per (view, ray) of the first round's partial sums (car_fused_samples_parts)
inline size_t step_groups(const car_dims& d) { const int ts = car_fused_tile_steps(); return (size_t)((d.P + ts - 1) / ts); }
Work work_layout(const car_dims& d) {
    Work w;
    Carver c(nullptr, kRound);
    auto take = [&](size_t n) { return Span{c.at<float>(n), n}; };
    const size_t n = (size_t)d.b * d.V, S = n * d.R * d.P, BR = (size_t)d.b * d.R;
    w.rays = take(n * d.R * CAR_RAY_FLOATS);
    w.phi_x = take(BR * kPhiLd);
    w.e = take(S * kC);
    w.g = take(S * CAR_G_DIM);
    w.logit = take(S);
    w.logit2 = take(S);
    w.pt = take(S * 3);
    w.pixel_val = take(S * 2);
    w.coords = take(n * d.R * 9);
    w.at_wt = take(S);
    w.at_wt2 = take(S);
    w.amax = take(n * d.R);
    w.depth = take(BR);
    w.ebar = take(BR * kC);
    w.z1 = take(BR * kE);
    w.uh = take(BR * kD);
    w.valid = take(BR);
    w.part = take(n * d.R * step_groups(d) * kC);
    w.total = c.bytes() / sizeof(float);
    return w;
}

// ---- stage timing --------------------------------------------------------------------------------------------------
struct StageRec { const char* name; hipEvent_t start, stop; };
struct Profile {
    bool on = false;
    std::vector<StageRec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t event() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) e = nullptr;
        return e;
    }
    void clear() {
        for (StageRec& r : recs) { pool.push_back(r.start); pool.push_back(r.stop); }
        recs.clear();
    }
};
thread_local Profile g_prof;
// brackets the launches of one stage with two events on the caller's stream (when profiling is on)
struct Stage {
    hipStream_t st;
    bool live;
    Stage(const char* name, hipStream_t s) : st(s), live(g_prof.on) {
        if (!live) return;
        StageRec r{name, g_prof.event(), g_prof.event()};
        if (!r.start || !r.stop) { live = false; return; }
        (void)hipEventRecord(r.start, st);
        g_prof.recs.push_back(r);
    }
    ~Stage() { if (live) (void)hipEventRecord(g_prof.recs.back().stop, st); }
};

}  // namespace

extern "C" void car_profile_enable(int on) { g_prof.clear(); g_prof.on = on != 0; }
extern "C" void car_profile_reset(void) { g_prof.clear(); }
extern "C" int car_profile_count(void) { return (int)g_prof.recs.size(); }
extern "C" int car_profile_read(int i, const char** name, float* ms) {
    CAR_REQUIRE(i >= 0 && i < (int)g_prof.recs.size() && name && ms, "car_profile_read: no stage %d", i);
    const StageRec& r = g_prof.recs[i];
    CAR_CHECK_HIP(hipEventSynchronize(r.stop), "car_profile_read: %s", hipGetErrorString(hipGetLastError()));
    CAR_CHECK_HIP(hipEventElapsedTime(ms, r.start, r.stop), "car_profile_read: %s", hipGetErrorString(hipGetLastError()));
    *name = r.name;
    return CAR_OK;
}

// torch.linspace (CPU, fp32): step = (b - a) / (n - 1); first half a + step * i, second half b - step * (n - 1 - i)
extern "C" void car_linspace(float a, float b, int n, float* out) {
    if (n == 1) { out[0] = a; return; }
    const float step = (b - a) / (float)(n - 1);
    const int half = n / 2;
    for (int i = 0; i < n; ++i) out[i] = i < half ? a + step * (float)i : b - step * (float)(n - 1 - i);
}

extern "C" size_t car_plan_bytes(const car_dims* dims) {
    if (check_dims(dims, "car_plan_bytes") != CAR_OK) return 0;
    return plan_layout(*dims).total * sizeof(float);
}
extern "C" size_t car_workspace_bytes(const car_dims* dims) {
    if (check_dims(dims, "car_workspace_bytes") != CAR_OK) return 0;
    return work_layout(*dims).total * sizeof(float);
}

namespace {
// the gmaps buffer (floats): the lattice, gmeta, then the projected levels (scratch of car_project_maps: the merge reads them)
struct Gmaps { size_t gmeta, level[CAR_MAX_LEVELS], total; };
Gmaps gmaps_layout(const car_dims& d) {
    Gmaps g{};
    Carver c(nullptr, kRound);
    const car_lattice L = car_lattice_of(d);
    c.at<float>((size_t)d.b * d.V * 2 * L.h * L.w * kC);
    g.gmeta = c.at<float>(64);
    for (int l = 0; l < d.n_levels; ++l) g.level[l] = c.at<float>((size_t)d.b * d.V * d.level_h[l] * d.level_w[l] * kC);
    g.total = c.bytes() / sizeof(float);
    return g;
}
}  // namespace
extern "C" size_t car_gmeta_offset(const car_dims* dims) {
    if (check_dims(dims, "car_gmeta_offset") != CAR_OK) return 0;
    return gmaps_layout(*dims).gmeta;
}
extern "C" size_t car_gmaps_floats(const car_dims* dims) {
    if (check_dims(dims, "car_gmaps_floats") != CAR_OK) return 0;
    return gmaps_layout(*dims).total;
}
extern "C" int car_lattice_shape(const car_dims* dims, int* lat_h, int* lat_w, int* lat_pad) {
    CAR_TRY(check_dims(dims, "car_lattice_shape"));
    CAR_REQUIRE(lat_h && lat_w && lat_pad, "car_lattice_shape: null pointer");
    const car_lattice L = car_lattice_of(*dims);
    *lat_h = L.h; *lat_w = L.w; *lat_pad = L.pad;
    return CAR_OK;
}
extern "C" int car_workspace_find(const car_dims* dims, const char* name, size_t* offset_floats, size_t* n_floats) {
    CAR_TRY(check_dims(dims, "car_workspace_find"));
    CAR_REQUIRE(name && offset_floats && n_floats, "car_workspace_find: null pointer");
    const Work w = work_layout(*dims);
    for (const auto& t : kFindable)
        if (strcmp(t.name, name) == 0) { *offset_floats = (w.*t.buf).off; *n_floats = (w.*t.buf).cnt; return CAR_OK; }
    car_set_error("car_workspace_find: unknown tensor '%s'", name);
    return CAR_E_ARG;
}

extern "C" int car_plan_build(const car_dims* dims, const car_weights* w, void* plan, void* stream) {
    CAR_TRY(check_dims(dims, "car_plan_build"));
    CAR_REQUIRE(w && plan, "car_plan_build: null pointer");
    const float* const* all = reinterpret_cast<const float* const*>(w);
    for (size_t k = 0; k < sizeof(car_weights) / sizeof(const float*); ++k)
        CAR_REQUIRE(all[k], "car_plan_build: weight pointer %zu of car_weights is null", k);
    CAR_REQUIRE(car_fused_blob_floats() == (size_t)kBlobTiles * kTile && car_fused_bias_floats() == (size_t)(kBiasFloats + kBiasScratch),
                "car_plan_build: the fused kernel was built with another weight layout");
    const Plan p = plan_layout(*dims);
    float* base = static_cast<float*>(plan);
    hipStream_t st = (hipStream_t)stream;
    // sample positions linspace(0, 1, P) with torch's CPU arithmetic (models.py:261)
    {
        float steps[1024];
        CAR_REQUIRE(dims->P <= 1024, "car_plan_build: P too large");
        car_linspace(0.0f, 1.0f, dims->P, steps);
        CAR_CHECK_HIP(hipMemcpyAsync(base + p.steps, steps, sizeof(float) * dims->P, hipMemcpyHostToDevice, st), "car_plan_build: upload failed: %s",
                      hipGetErrorString(hipGetLastError()));
        CAR_CHECK_HIP(hipStreamSynchronize(st), "car_plan_build: upload failed: %s", hipGetErrorString(hipGetLastError()));
    }
    // split-fp16 operand tiles of the fused per-sample kernel and of the round-2 kernel
    CAR_TRY(car_fused_pack(w, base + p.blob, base + p.fbias, base + p.wpt, stream));
    CAR_TRY(car_round2q_pack(w->query_repeat_embed_w, w->query_repeat_embed_b, w->query_repeat_embed_2_w, w->query_repeat_embed_2_b,
                             w->query_embed_w, w->query_embed_b, w->query_embed_2_w, w->query_embed_2_b, base + p.r2qw, base + p.r2qb, stream));
    // fp32 MFMA layers (car_linear.hip)
    int coff = 0;
    for (int l = 0; l < dims->n_levels; ++l) {
        CAR_TRY(car_linear_pack(w->query_encode_latent_w + coff, kC + 3, nullptr, dims->level_c[l], kC, base + p.proj[l], stream));
        if (level_on_f16_pipe(dims->level_c[l]))
            CAR_TRY(car_linear_x3_pack(w->query_encode_latent_w + coff, kC + 3, dims->level_c[l], kC, base + p.proj16[l], stream));
        coff += dims->level_c[l];
    }
    // the per-ray chains (car_raychain.hip), split-fp16 tiles: where each layer of car_chain_layout.h's table finds its weight rows, their
    // stride and its bias
    struct { const float* W; int ldw; const float* bias; } src[kChainLayers];
    src[kSlotLatentValue] = {w->latent_value_w, kC, w->latent_value_b};
    src[kSlotEncodeLatent] = {w->encode_latent_w, kE, w->encode_latent_b};
    src[kSlotQueryRepeat] = {w->query_repeat_embed_w, kD + 16, nullptr};
    src[kSlotLinIn] = {w->phi_lin_in_w, kPhiIn, w->phi_lin_in_b};
    for (int i = 0; i < kBlocks; ++i) {
        src[chain_block_slot(i, 0)] = {w->phi_lin_z_w[i], 2 * kE, w->phi_lin_z_b[i]};
        src[chain_block_slot(i, 1)] = {w->phi_fc_0_w[i], kD, w->phi_fc_0_b[i]};
        src[chain_block_slot(i, 2)] = {w->phi_fc_1_w[i], kD, w->phi_fc_1_b[i]};
    }
    src[kSlotLinOut] = {w->phi_lin_out_w, kD, w->phi_lin_out_b};
    for (int slot = 0; slot < kChainLayers; ++slot) {
        const ChainLayer& L = kChainLayer[slot];
        CAR_TRY(car_chain_pack(src[slot].W, src[slot].ldw, L.halves ? src[slot].W + L.K : nullptr, L.K, L.N, L.chained, base + p.chain[slot],
                               base + p.chain_scale, slot, stream));
    }
    CAR_CHECK_HIP(hipMemsetAsync(base + p.tail_bias, 0, sizeof(float) * kTailBiasFloats, st), "car_plan_build: memset failed");
    auto biases = [&](float* table, const int* seq, int n) {
        for (int pos = 0; pos < n; ++pos)
            if (kChainLayer[seq[pos]].bias)
                CAR_CHECK_HIP(hipMemcpyAsync(table + chain_bias_at(seq, pos), src[seq[pos]].bias, sizeof(float) * kChainLayer[seq[pos]].N, hipMemcpyDeviceToDevice, st),
                              "car_plan_build: bias copy failed");
        return CAR_OK;
    };
    CAR_TRY(biases(base + p.mid_bias, kMidSeq, kMidLayers));
    CAR_TRY(biases(base + p.tail_bias, kTailSeq, kTailLayers));
    return CAR_OK;
}

// ---- the fp16 precision's plan (car_plan_f16_*): the fused kernel's compact blob, its bias table and point table ----------
struct Plan16 { size_t blob, fbias, wpt, total; };                 // offsets in floats
Plan16 plan16_layout() {
    Carver c(nullptr, kRound);
    return {c.at<float>(car_fused_blob16_floats()), c.at<float>(car_fused_bias_floats()), c.at<float>((size_t)kC * 4), c.bytes() / sizeof(float)};
}
extern "C" size_t car_plan_f16_bytes(const car_dims* dims) {
    if (check_dims(dims, "car_plan_f16_bytes") != CAR_OK) return 0;
    return plan16_layout().total * sizeof(float);
}
extern "C" int car_plan_f16_build(const car_dims* dims, const car_weights* w, void* plan16, void* stream) {
    CAR_TRY(check_dims(dims, "car_plan_f16_build"));
    CAR_REQUIRE(w && plan16, "car_plan_f16_build: null pointer");
    CAR_REQUIRE(car_fused_blob16_floats() == (size_t)kBlobTiles * kTileHi && car_fused_bias_floats() == (size_t)(kBiasFloats + kBiasScratch),
                "car_plan_f16_build: the fused kernel was built with another weight layout");
    const Plan16 p = plan16_layout();
    float* base = static_cast<float*>(plan16);
    return car_fused_pack_hi(w, base + p.blob, base + p.fbias, base + p.wpt, stream);
}

extern "C" int car_project_maps(const car_dims* dims, const void* plan, const float* const* maps, float* gmaps, void* stream) {
    CAR_TRY(check_dims(dims, "car_project_maps"));
    CAR_REQUIRE(plan && maps && gmaps, "car_project_maps: null pointer");
    const Plan p = plan_layout(*dims);
    const float* base = static_cast<const float*>(plan);
    hipStream_t st = (hipStream_t)stream;
    const Gmaps gm = gmaps_layout(*dims);
    float* gmeta = gmaps + gm.gmeta;
    CAR_CHECK_HIP(hipMemsetAsync(gmeta, 0, sizeof(float) * CAR_MAX_LEVELS, st), "car_project_maps: memset failed");
    const car_lattice L = car_lattice_of(*dims);
    const float* lv[CAR_MAX_LEVELS];
    for (int l = 0; l < dims->n_levels; ++l) {
        CAR_REQUIRE(maps[l], "car_project_maps: level %d is null", l);
        const long M = (long)dims->b * dims->V * dims->level_h[l] * dims->level_w[l];
        float* gl = gmaps + gm.level[l];
        // G_l = W1[:, ch_l] F_l per texel: on the f16 matrix pipe with fp16 hi / lo operand halves (car_linear_x3: fp32-class accuracy at
        // 2.3x the fp32 pipe's rate — the arithmetic of the staged route's engine._projected_maps) where the level's width allows it
        if (level_on_f16_pipe(dims->level_c[l]) && ((uintptr_t)maps[l] & 15) == 0)
            CAR_TRY(car_linear_x3(maps[l], dims->level_c[l], base + p.proj16[l], nullptr, dims->level_c[l], kC, gl, kC, M, 0, stream));
        else
            CAR_TRY(car_linear(maps[l], dims->level_c[l], base + p.proj[l], dims->level_c[l], kC, gl, kC, M, 0, stream));
        lv[l] = gl;
    }
    // the lattice, and in the same pass its largest magnitude (gmeta[0], zeroed above): it bounds h (the fused kernel scales its fp16
    // operands by it)
    return car_launch_merge(lv, dims->level_h, dims->level_w, L.r, dims->n_levels, L.h, L.w, L.pad, dims->b * dims->V, gmaps,
                            reinterpret_cast<unsigned*>(gmeta), st, "car_project_maps (merge)");
}

// the launches of one forward call in two phases: CAR_PHASE_SAMPLES = rays + the fused per-sample kernel (compute / power bound),
// CAR_PHASE_RAYS = the attention rounds and the per-ray chains (HBM bound), which only read what the first phase left in the workspace
// plan16 (car_plan_f16_build) non-null: the fused kernel's fp16 instance; every other launch is the fp32 route's own
// entry: the C entry's name, for the message about `phases`
static int render_phases(const char* entry, const car_dims* dims, const void* plan, const car_inputs* in, const car_outputs* out,
                         void* workspace, size_t workspace_bytes, int phases, void* stream, const void* plan16 = nullptr) {
    const int which = phases & ~(CAR_PHASE_ROWS_FIRST_ROUND | CAR_PHASE_SPLIT_SECOND_ROUND);
    CAR_REQUIRE(which == CAR_PHASE_SAMPLES || which == CAR_PHASE_RAYS || which == (CAR_PHASE_SAMPLES | CAR_PHASE_RAYS),
                "%s: phases = %d (CAR_PHASE_SAMPLES, CAR_PHASE_RAYS or both, optionally | CAR_PHASE_ROWS_FIRST_ROUND | CAR_PHASE_SPLIT_SECOND_ROUND)",
                entry, phases);
    CAR_TRY(check_dims(dims, "car_render_forward"));
    CAR_REQUIRE(plan && in && out && workspace, "car_render_forward: null pointer");
    CAR_REQUIRE(in->poses && in->uv && in->lattice && in->gmeta && out->rgb, "car_render_forward: poses, uv, lattice, gmeta and rgb are required");
    const car_dims& d = *dims;
    const Plan p = plan_layout(d);
    const Work w = work_layout(d);
    CAR_REQUIRE(workspace_bytes >= w.total * sizeof(float), "car_render_forward: workspace of %zu bytes, %zu needed", workspace_bytes,
                w.total * sizeof(float));
    const float* pl = static_cast<const float*>(plan);
    float* ws = static_cast<float*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const int b = d.b, V = d.V, R = d.R, P = d.P;
    const bool rows_first = (phases & CAR_PHASE_ROWS_FIRST_ROUND) != 0;
    CAR_REQUIRE(!d.no_sample || in->steps, "car_render_forward: no_sample needs `steps` (the P depths along the query ray, models.py:221-222)");
    const float* steps = in->steps ? in->steps : pl + p.steps;
    const long BR = (long)b * R;
    float* coords = out->coords ? out->coords : ws + w.coords.off;
    float* pixel_val = out->pixel_val ? out->pixel_val : ws + w.pixel_val.off;
    float* at_wt = out->at_wt ? out->at_wt : ws + w.at_wt.off;
    float* depth = out->depth_ray ? out->depth_ray : ws + w.depth.off;
    float* valid = out->valid_mask ? out->valid_mask : ws + w.valid.off;
    int32_t* amax = out->at_wt_max ? out->at_wt_max : reinterpret_cast<int32_t*>(ws + w.amax.off);

    if (phases & CAR_PHASE_SAMPLES) {
    {   // a4-a6: rays, their epipolar segments, the decoder's ray input (columns 18, 19 of phi_x stay zero)
        Stage stage("ray_setup", st);
        CAR_CHECK_HIP(hipMemsetAsync(ws + w.phi_x.off, 0, sizeof(float) * BR * kPhiLd, st), "car_render_forward: memset failed");
        CAR_TRY(car_ray_setup(in->poses, in->uv, b, V, R, d.H, d.W, P, d.no_sample != 0, steps, ws + w.rays.off, coords, ws + w.phi_x.off, kPhiLd, stream));
    }
    {   // a6-a13 + round-1 logits: the fused per-sample kernel
        Stage stage("fused_samples", st);
        const car_lattice L = car_lattice_of(d);
        if (plan16) {
            const Plan16 q = plan16_layout();
            const float* p16 = static_cast<const float*>(plan16);
            CAR_TRY(car_fused_samples_f16(in->poses, ws + w.rays.off, steps, in->lattice, L.h, L.w, L.pad, in->gmeta, p16 + q.wpt, p16 + q.blob,
                                          p16 + q.fbias, b, V, R, P, d.H, d.W, d.no_sample != 0, ws + w.e.off, ws + w.g.off, ws + w.logit.off, ws + w.pt.off, pixel_val,
                                          rows_first ? nullptr : ws + w.part.off, stream));
        } else if (rows_first)
            CAR_TRY(car_fused_samples(in->poses, ws + w.rays.off, steps, in->lattice, L.h, L.w, L.pad, in->gmeta, pl + p.wpt, pl + p.blob,
                                      pl + p.fbias, b, V, R, P, d.H, d.W, d.no_sample != 0, ws + w.e.off, ws + w.g.off, ws + w.logit.off, ws + w.pt.off, pixel_val, stream));
        else
            CAR_TRY(car_fused_samples_parts(in->poses, ws + w.rays.off, steps, in->lattice, L.h, L.w, L.pad, in->gmeta, pl + p.wpt, pl + p.blob,
                                            pl + p.fbias, b, V, R, P, d.H, d.W, d.no_sample != 0, ws + w.e.off, ws + w.g.off, ws + w.logit.off, ws + w.pt.off, pixel_val,
                                            ws + w.part.off, stream));
    }
    }
    if (!(phases & CAR_PHASE_RAYS)) return CAR_OK;
    {   // a14 + a16: attention round 1, depth read-out, argmax.  The value average comes from the per-step-group partial sums the
        // fused kernel left behind (an eighth of the rows of e), so e itself is streamed from HBM by the second round only
        Stage stage("attend_1", st);
        if (rows_first)
            CAR_TRY(car_attend(ws + w.logit.off, nullptr, kD, ws + w.e.off, kC, b, V, R, P, nullptr, 0.0f, at_wt, ws + w.ebar.off, kC, 1, ws + w.pt.off, in->poses,
                               depth, amax, stream));
        else
            CAR_TRY(car_attend_parts(ws + w.logit.off, ws + w.part.off, car_fused_tile_steps(), kC, b, V, R, P, at_wt, ws + w.ebar.off, kC, 1, ws + w.pt.off, in->poses,
                                     depth, amax, stream));
    }
    // weight-chunk tables of the two per-ray chains (car_raychain.hip): float offset inside the plan and tile count of every chunk of
    // the sequence's layers, in the order the kernel consumes them
    unsigned offs[kMaxChunks];
    int nts[kMaxChunks];
    auto chunks = [&](const int* seq, int n) {
        int nch = 0;
        for (int i = 0; i < n; ++i)
            for (int c = 0, nt = chain_tiles(seq[i]); c < chain_chunks(seq[i]); ++c) { offs[nch] = (unsigned)(p.chain[seq[i]] + (size_t)c * nt * kTileFloats); nts[nch++] = nt; }
        return nch;
    };
    CAR_REQUIRE(p.total < (1ull << 32), "car_render_forward: plan too large");
    if (d.repeat_attention) {
        {   // a15, per ray: z1 = Wv ebar + bv; uh = Wr1[:, :128] encode_latent(z1)
            Stage stage("ray_layers_1", st);
            const int nch = chunks(kMidSeq, kMidLayers);
            CAR_TRY(car_ray_mid(pl, offs, nts, nch, pl + p.mid_bias, pl + p.chain_scale, kMidSeq, kMidLayers, ws + w.ebar.off, kC, ws + w.z1.off, ws + w.uh.off, BR, stream));
        }
        if (!(phases & CAR_PHASE_SPLIT_SECOND_ROUND) && car_attend_round2_supports(kC, V, P)) {
            // a15 per sample + the second round's softmax and value average in one launch: the logits are made on the matrix pipe under the
            // stream of e and never reach memory (car_round2_attend.hip; the workspace keeps its logit2 slot, unused here)
            Stage stage("attend_2", st);
            CAR_TRY(car_attend_round2(ws + w.g.off, ws + w.uh.off, pl + p.r2qw, pl + p.r2qb, ws + w.e.off, kC, b, V, R, P, ws + w.at_wt2.off, ws + w.ebar.off, kC,
                                      nullptr, stream));
        } else {
            {   // a15, per sample: second-round query and logits
                Stage stage("round2_logits", st);
                // no 128-wide query rows exist on this route: <q2, qry> is a bilinear form of two hidden vectors both made from g (car_round2.hip)
                CAR_TRY(car_round2_logits_from_g(ws + w.g.off, ws + w.uh.off, pl + p.r2qw, pl + p.r2qb, b, V, R, P, ws + w.logit2.off, stream));
            }
            {
                Stage stage("attend_2", st);
                CAR_TRY(car_attend(ws + w.logit2.off, nullptr, kD, ws + w.e.off, kC, b, V, R, P, nullptr, 0.0f, ws + w.at_wt2.off, ws + w.ebar.off, kC, 1, nullptr,
                                   nullptr, nullptr, nullptr, stream));
            }
        }
    } else                                                                                          // no second round: z = Wv ebar1 + bv
        CAR_CHECK_HIP(hipMemsetAsync(ws + w.z1.off, 0, sizeof(float) * BR * kE, st), "car_render_forward: memset failed");
    {   // z = (Wv ebar + bv) + V z1 (models.py:561-565), light-field decoder (resnet_block_fc.py:132-168), valid mask / white background
        Stage stage("ray_layers_2", st);
        const int nch = chunks(kTailSeq, kTailLayers);
        CAR_TRY(car_ray_tail(pl, offs, nts, nch, pl + p.tail_bias, pl + p.chain_scale, kTailSeq, kTailLayers, ws + w.ebar.off, kC, ws + w.phi_x.off, kPhiLd, ws + w.z1.off,
                             ws + w.rays.off, b, V, R, out->rgb, valid, stream));
    }
    return CAR_OK;
}

extern "C" int car_render_forward(const car_dims* dims, const void* plan, const car_inputs* in, const car_outputs* out,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    return render_phases("car_render_forward", dims, plan, in, out, workspace, workspace_bytes, CAR_PHASE_SAMPLES | CAR_PHASE_RAYS, stream);
}

extern "C" int car_render_forward_phase(const car_dims* dims, const void* plan, const car_inputs* in, const car_outputs* out,
                                        void* workspace, size_t workspace_bytes, int phases, void* stream) {
    return render_phases("car_render_forward_phase", dims, plan, in, out, workspace, workspace_bytes, phases, stream);
}

// The opt-in fp16 precision of the same forward: the fused per-sample kernel takes one product per term from plan16 (car_plan_f16_build);
// plan still supplies the sample positions, the round-2 packing and the per-ray chains.  Phases and flags as car_render_forward_phase.
extern "C" int car_render_forward_f16(const car_dims* dims, const void* plan, const void* plan16, const car_inputs* in, const car_outputs* out,
                                      void* workspace, size_t workspace_bytes, int phases, void* stream) {
    CAR_REQUIRE(plan16, "car_render_forward_f16: null plan16");
    return render_phases("car_render_forward_f16", dims, plan, in, out, workspace, workspace_bytes, phases, stream, plan16);
}
