// Executor of libmetro_hip.so: runs the layer list planner.cpp built -- one launch per layer, eagerly or as a captured hipGraph.
#include <cstring>
#include <string>
#include <vector>

#include "plan.h"

using namespace metro;

namespace {

// One layer of the plan at batch n.  `dump` (metro_forward_upto stopping at this layer): launches whose intermediate tensors live on
// chip also write them out -- the fp32 logits of the one-launch head, conv1's output of a conv1+conv2 launch.
// `coords01` (optional): the finalize launch also writes the soft-argmax coordinates in [0,1] there (metro_forward_coords01).
// `images_u8` (metro_forward_u8): `images` points to uint8 crops; the layer that reads them runs the uint8 form of its kernel.
// `mo` (metro_forward_moments): its scratch selects the MOMENTS instantiations of the head / soft-argmax launches.
// `head_logits` (a forward with heat-map, mode or prior buffers bound): where the one-launch head also writes its fp32 logits, as for a dump.
int launch_layer(const MetroPlan* p, const char* d_params, int li, const float* images, int n, float* poses, char* ws, hipStream_t stream, bool dump,
                 float* coords01 = nullptr, bool images_u8 = false, const MomentsOut& mo = MomentsOut{}, float* head_logits = nullptr) {
    const Layer& L = p->layers[li];
    auto slot_ptr = [&](int slot) -> void* {
        if (slot == S_IMAGES) return const_cast<float*>(images);
        if (slot < 0) return nullptr;
        return ws + p->slot_offset[slot];
    };
    auto prm = [&](int idx) -> const void* { return idx < 0 ? nullptr : d_params + p->params[idx].offset; };
    switch (L.kind) {
        case LK_PREP:
            if (images_u8)
                return launch_prep_input_u8_f16(reinterpret_cast<const unsigned char*>(images), n, p->spec.proc_side, slot_ptr(L.out_slot), stream);
            return launch_prep_input_f16(images, n, p->spec.proc_side, slot_ptr(L.out_slot), stream);
        case LK_POOL:
            return launch_maxpool(slot_ptr(L.in_slot), slot_ptr(L.out_slot), n, L.cd.h_in, L.cd.w_in, L.cd.c_in, p->act_dtype, stream);
        case LK_CONV: {
            MetroConvDesc cd = L.cd;
            cd.n = n;
            auto fprm = [&](int idx) { return static_cast<const float*>(prm(idx)); };
            void* in = slot_ptr(L.in_slot);
            void* out = slot_ptr(L.out_slot);
            const void* w = prm(L.main.w);
            const float* bias = fprm(L.main.bias);
            ConvFused f;
            switch (L.form) {
                case LayerForm::Head: {
                    float* logits_dump = dump ? static_cast<float*>(out) : head_logits;
                    return launch_head_f16(in, w, bias, prm(L.main.scale), prm(L.main.shift), n, L.cd.c_in, L.cd.c_out, p->spec.n_joints_head,
                                           p->spec.depth, L.cd.h_in, static_cast<float*>(slot_ptr(S_PART)), logits_dump, stream,
                                           static_cast<float*>(mo.scratch));
                }
                case LayerForm::StemPoolF32In:
                    if (images_u8)
                        return launch_stem_pool_u8in(reinterpret_cast<const unsigned char*>(images), w, bias, out, n, p->spec.proc_side, stream);
                    return launch_stem_pool_f32in(images, w, bias, out, n, p->spec.proc_side, stream);
                case LayerForm::StemPool:
                    return launch_stem_pool_f16(in, w, bias, out, n, p->spec.proc_side, stream);
                case LayerForm::Conv1Conv2: {
                    ConvPre1 p1;
                    p1.w1 = prm(L.conv1.w); p1.bias1 = fprm(L.conv1.bias);
                    p1.pro_scale = prm(L.conv1.scale); p1.pro_shift = prm(L.conv1.shift);
                    p1.t1_dump = dump ? slot_ptr(S_T1) : nullptr;        // conv1's output exists in LDS only; layer dumps get a copy
                    return launch_conv3x3_c64(cd, in, w, bias, out, stream, &p1);
                }
                case LayerForm::Plain:
                    if (p->fast)
                        return launch_conv_f16(cd, {in, w, bias, prm(L.main.scale), prm(L.main.shift), slot_ptr(L.res_slot), out}, stream);
                    if (p->spec.precision == METRO_PREC_F32M)
                        return launch_conv_f32m(cd, in, static_cast<const float*>(w), bias, fprm(L.main.scale), fprm(L.main.shift),
                                                slot_ptr(L.res_slot), out, stream);
                    return launch_conv_f64acc(cd, in, static_cast<const double*>(w), static_cast<const double*>(prm(L.main.bias)),
                                              static_cast<const double*>(prm(L.main.scale)), static_cast<const double*>(prm(L.main.shift)),
                                              slot_ptr(L.res_slot), out, stream);
                case LayerForm::Pair:
                    f.form = ConvForm::Pair;
                    f.pair = {L.cd.c_out - L.c2, L.c2, 1, slot_ptr(L.out2_slot)};
                    return launch_conv_f16(cd, {in, w, bias, prm(L.main.scale), prm(L.main.shift), nullptr, out}, stream, f);
                case LayerForm::Next:
                case LayerForm::NextProj:
                case LayerForm::NextRebuild:
                    f.form = conv_form(L.form);
                    f.next = {prm(L.next.w), fprm(L.next.bias), prm(L.next.scale), prm(L.next.shift), slot_ptr(L.out2_slot), L.c2};
                    if (f.form != ConvForm::Next)
                        f.psc = {slot_ptr(L.psc_slot), prm(L.psc.w), fprm(L.psc.bias), prm(L.psc.scale), prm(L.psc.shift)};
                    if (f.form == ConvForm::NextRebuild) {
                        f.rb.t2_prev = slot_ptr(L.reb_slot); f.rb.w3_prev = prm(L.reb.w); f.rb.bias3_prev = fprm(L.reb.bias);
                    }
                    // block1 without its residual stream in HBM: metro_forward_upto stopping here (dump) stores the sum in full, on the
                    // classic kernel
                    f.rb.out_mode = dump ? 0 : L.out_mode;
                    f.rb.classic = dump ? 1 : 0;
                    if (f.rb.out_mode == 2) { f.rb.out_sub = slot_ptr(L.sub_slot); f.rb.sub_off = L.sub_off; f.rb.h_sub = f.rb.w_sub = L.sub_side; }
                    return launch_conv_f16(cd, {in, w, bias, nullptr, nullptr, slot_ptr(L.res_slot), out}, stream, f);
            }
            break;
        }
        case LK_SOFTARGMAX: {
            if (poses == nullptr) { set_error("metro_forward: poses_out is NULL"); return METRO_ERR_INVALID_ARG; }
            const SoftArgmaxArgs a = make_softargmax_args(p->spec, n);
            if (L.form == LayerForm::Head)
                return launch_softargmax_finalize(static_cast<const float*>(slot_ptr(S_PART)), a,
                                                  head_f16_records(n, L.head_c_in, a.depth * a.n_joints_head, a.side), poses, stream, coords01,
                                                  static_cast<int32_t*>(slot_ptr(S_STATUS)), mo);
            // precise: 0 fp32 / fp32, 1 fp32 logits + fp64 accumulators (F32 and F32M modes), 2 fp64 / fp64
            return launch_softargmax(slot_ptr(L.in_slot), a, p->spec.precision == METRO_PREC_F32M ? 1 : p->spec.precision, slot_ptr(S_PART), poses, stream,
                                     coords01, static_cast<int32_t*>(slot_ptr(S_STATUS)), mo);
        }
    }
    set_error("internal: layer %d has unknown kind %d", li, L.kind);
    return METRO_ERR_STATE;
}

int run_layers(MetroPlan* p, const float* images, int n, float* poses, void* ws_, hipStream_t stream,
               int last_layer, float* ms_out, float* coords01 = nullptr, bool images_u8 = false, const MomentsOut& mo = MomentsOut{}) {
    METRO_CHECK_ARG(p != nullptr, "plan is NULL");
    METRO_CHECK_ARG(n > 0 && n <= p->max_batch, "batch %d outside [1, %d]", n, p->max_batch);
    METRO_CHECK_ARG(images != nullptr && ws_ != nullptr, "NULL images/workspace pointer");
    if (p->d_params == nullptr) { set_error("metro_forward: parameters not bound (metro_plan_bind_params)"); return METRO_ERR_STATE; }
    char* ws = static_cast<char*>(ws_);
    const int nl = (int)p->layers.size();
    if (last_layer < 0 || last_layer >= nl) last_layer = nl - 1;
    // heat-map buffers bound (metro_plan_bind_heatmaps): a forward that runs the whole plan also writes the marginals
    const bool heat = p->heat.scratch != nullptr && last_layer == nl - 1;
    const int side = p->spec.proc_side / p->spec.stride;
    METRO_CHECK_ARG(!heat || n <= p->heat.max_n, "batch %d exceeds the %d crops the bound heat-map buffers hold (metro_plan_bind_heatmaps)",
                    n, p->heat.max_n);
    // mode buffers bound (metro_plan_bind_modes): the same; the head's one logits store goes to the heat-map scratch when both are bound
    const bool modes = p->modes.scratch != nullptr && last_layer == nl - 1;
    METRO_CHECK_ARG(!modes || n <= p->modes.max_n, "batch %d exceeds the %d crops the bound mode buffers hold (metro_plan_bind_modes)",
                    n, p->modes.max_n);
    // prior buffers bound (metro_plan_bind_prior): the same; the logits store goes to the heat-map scratch, else to the modes', else here
    const bool prior = p->prior.scratch != nullptr && last_layer == nl - 1;
    METRO_CHECK_ARG(!prior || n <= p->prior.max_n, "batch %d exceeds the %d crops the bound prior buffers hold (metro_plan_bind_prior)",
                    n, p->prior.max_n);
    // a track table bound (metro_plan_bind_track_prior): the prior rows are written behind the finalize launch, the posterior follows
    const bool track = p->track.scratch != nullptr && last_layer == nl - 1;
    METRO_CHECK_ARG(!track || n <= p->track.max_n, "batch %d exceeds the %d crops the bound track-prior buffers hold (metro_plan_bind_track_prior)",
                    n, p->track.max_n);
    METRO_CHECK_ARG(!track || p->track.params.depth != METRO_TRACK_PRIOR_DEPTH_ROOT || coords01 != nullptr,
                    "METRO_TRACK_PRIOR_DEPTH_ROOT is bound (metro_plan_bind_track_prior): the forward needs a coords01 output "
                    "(metro_forward_coords01, metro_forward_u8 or metro_forward_moments with one)");
    // a view fusion bound (metro_plan_bind_view_fusion): the last launches of the forward; without the caller's centres the
    // triangulation reads this forward's own coords01 (and cov01 under METRO_TRI_COVARIANCE)
    const bool fusion = p->fusion.points != nullptr && last_layer == nl - 1;
    METRO_CHECK_ARG(!fusion || n <= p->fusion.max_n, "batch %d exceeds the %d crops the bound view-fusion buffers hold (metro_plan_bind_view_fusion)",
                    n, p->fusion.max_n);
    METRO_CHECK_ARG(!fusion || p->fusion.centres != nullptr || coords01 != nullptr,
                    "a view fusion without centres is bound (metro_plan_bind_view_fusion): the forward needs a coords01 output "
                    "(metro_forward_coords01, metro_forward_u8 or metro_forward_moments with one)");
    METRO_CHECK_ARG(!fusion || p->fusion.centres != nullptr || p->fusion.params.weights != METRO_TRI_COVARIANCE || mo.cov01 != nullptr,
                    "a view fusion without centres is bound with METRO_TRI_COVARIANCE (metro_plan_bind_view_fusion): the forward needs "
                    "a cov01 output (metro_forward_moments with one)");
    // a skeleton bound (metro_plan_bind_skeleton_modes): one launch behind the modes', on whatever mode buffers it was given
    const bool skel = p->skel.prob != nullptr && last_layer == nl - 1;
    METRO_CHECK_ARG(!skel || n <= p->skel.max_n, "batch %d exceeds the %d crops the bound skeleton buffers hold (metro_plan_bind_skeleton_modes)",
                    n, p->skel.max_n);
    METRO_CHECK_ARG(!skel || p->skel.coords01_sel == nullptr || coords01 != nullptr,
                    "a coords01_sel output is bound (metro_plan_bind_skeleton_modes): the forward needs a coords01 output "
                    "(metro_forward_coords01, metro_forward_u8 or metro_forward_moments with one)");
    float* head_logits = nullptr;
    if (heat && p->head_fused)
        head_logits = heat_marginals_scratch_logits(p->heat.scratch, p->heat.max_n, side, p->spec.n_joints_head, p->spec.depth);
    else if (modes && p->head_fused)
        head_logits = static_cast<float*>(p->modes.scratch);
    else if (prior && p->head_fused)
        head_logits = static_cast<float*>(p->prior.scratch);
    else if (track && p->head_fused)
        head_logits = static_cast<float*>(p->track.scratch);

    std::vector<hipEvent_t> ev;
    if (ms_out) {
        ev.resize(2 * (last_layer + 1));
        for (auto& e : ev) METRO_HIP_CHECK(hipEventCreate(&e));
    }
    int st = METRO_OK;
    for (int li = 0; li <= last_layer && st == METRO_OK; ++li) {
        if (ms_out) METRO_HIP_CHECK(hipEventRecord(ev[2 * li], stream));
        st = launch_layer(p, p->d_params, li, images, n, poses, ws, stream, li == last_layer && li + 1 < nl, coords01, images_u8, mo, head_logits);
        if (ms_out) METRO_HIP_CHECK(hipEventRecord(ev[2 * li + 1], stream));
    }
    if (heat && st == METRO_OK)
        st = launch_heat_marginals(head_logits ? head_logits : static_cast<void*>(ws + p->slot_offset[S_LOGITS]),
                                   p->spec.precision == METRO_PREC_F32M ? 1 : p->spec.precision, n, p->heat.max_n, p->spec, p->heat.scratch,
                                   p->heat.xy, p->heat.z, stream);
    if (modes && st == METRO_OK)
        st = launch_heat_modes(head_logits ? head_logits : static_cast<void*>(ws + p->slot_offset[S_LOGITS]),
                               p->spec.precision == METRO_PREC_F32M ? 1 : p->spec.precision, n, p->modes.max_n, p->spec, p->modes.k,
                               p->modes.radius, p->modes.voxel, p->modes.stats, stream);
    if (skel && st == METRO_OK)
        st = launch_skeleton_modes(p->skel.voxel, p->skel.stats, p->skel.k, p->skel.lengths, p->skel.edges, p->skel.n_edges, p->skel.parent,
                                   p->skel.parent_edge, p->skel.params, coords01, n, p->skel.max_n, p->spec, p->skel.prob, p->skel.choice,
                                   p->skel.info, p->skel.coords01_sel, stream);
    if (prior && st == METRO_OK)
        st = launch_heat_posterior(head_logits ? head_logits : static_cast<void*>(ws + p->slot_offset[S_LOGITS]),
                                   p->spec.precision == METRO_PREC_F32M ? 1 : p->spec.precision, n, p->prior.max_n, p->spec, p->prior.prior,
                                   p->prior.post, stream);
    if (track && st == METRO_OK)
        st = launch_track_priors(p->track.state, p->track.capacity, p->track.slot, p->track.times, p->track.records, p->track.mirror,
                                 p->track.params, coords01, n, p->spec, p->track.prior, p->track.reason, stream);
    if (track && st == METRO_OK)
        st = launch_heat_posterior(head_logits ? head_logits : static_cast<void*>(ws + p->slot_offset[S_LOGITS]),
                                   p->spec.precision == METRO_PREC_F32M ? 1 : p->spec.precision, n, p->track.max_n, p->spec, p->track.prior,
                                   p->track.post, stream);
    // the triangulation's n_rays and residual pass through info and stats, which the fusion launch overwrites
    if (fusion && p->fusion.centres == nullptr && p->fusion.n_persons > 0 && st == METRO_OK)
        st = launch_triangulate_joints(coords01, p->fusion.params.weights == METRO_TRI_COVARIANCE ? mo.cov01 : nullptr, p->fusion.records, n,
                                       p->fusion.rows, p->fusion.n_rows, p->fusion.starts, p->fusion.n_persons, p->spec, p->fusion.mirror,
                                       p->fusion.params.weights, p->fusion.params.min_det, p->fusion.centres_out, p->fusion.info,
                                       p->fusion.stats, nullptr, stream);
    if (fusion && st == METRO_OK)
        st = launch_view_fusion(p->fusion.xy, p->fusion.records, p->fusion.rows, p->fusion.n_rows, p->fusion.starts, p->fusion.n_persons,
                                p->fusion.mirror, p->fusion.centres, p->fusion.params, n, p->spec, p->fusion.points, p->fusion.cov,
                                p->fusion.stats, p->fusion.info, p->fusion.centres_out, stream);
    if (ms_out) {
        if (st == METRO_OK) {
            METRO_HIP_CHECK(hipEventSynchronize(ev.back()));
            for (int li = 0; li <= last_layer; ++li) {
                float ms = 0.f;
                METRO_HIP_CHECK(hipEventElapsedTime(&ms, ev[2 * li], ev[2 * li + 1]));
                ms_out[li] += ms;
            }
        }
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    return st;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
extern "C" {

int metro_plan_layer_kernel(const MetroPlan* plan, int32_t index, int32_t n, char* buf, int32_t buf_len) {
    METRO_CHECK_ARG(plan && buf && buf_len > 1 && index >= 0 && index < (int)plan->layers.size(), "metro_plan_layer_kernel: bad argument");
    METRO_CHECK_ARG(n > 0 && n <= plan->max_batch, "metro_plan_layer_kernel: batch %d outside [1, %d]", n, plan->max_batch);
    // dry run of the layer's dispatch: the leaf launcher records the instantiation it would launch and returns
    KernelNotes& kn = kernel_notes();
    const int saved_mode = kn.mode;
    const std::string saved_ids(kn.ids);              // what the string holds, not its 4 KiB: this entry is called a million times per scan
    kn.mode = 2; kn.ids[0] = 0;
    static const char fake = 0;                       // pointers are never dereferenced in a dry run (launch_status asserts it)
    float dummy_poses = 0.f;
    const int st = launch_layer(plan, &fake, index, reinterpret_cast<const float*>(&fake), n, &dummy_poses,
                                const_cast<char*>(&fake), nullptr, false);
    snprintf(buf, (size_t)buf_len, "%s", kn.ids);
    kn.mode = saved_mode;
    memcpy(kn.ids, saved_ids.c_str(), saved_ids.size() + 1);
    return st;
}

int metro_plan_bind_params(MetroPlan* plan, const void* d_param_blob) {
    METRO_CHECK_ARG(plan && d_param_blob, "metro_plan_bind_params: NULL argument");
    METRO_CHECK_ARG(((uintptr_t)d_param_blob & 255) == 0, "parameter blob must be 256-byte aligned");
    plan->d_params = static_cast<const char*>(d_param_blob);
    // captured forwards bake the OLD blob's pointers into their kernel arguments: drop them
    for (GraphEntry& g : plan->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    plan->graphs.clear();
    return METRO_OK;
}

int64_t metro_plan_heatmaps_scratch_bytes(const MetroPlan* plan, int32_t max_n) {
    if (plan == nullptr || max_n < 1 || max_n > plan->max_batch) return -1;
    return heat_marginals_scratch_bytes(max_n, plan->spec.proc_side / plan->spec.stride, plan->spec.n_joints_head, plan->spec.depth,
                                        plan->head_fused);
}

int metro_plan_bind_heatmaps(MetroPlan* plan, float* d_xy_out, float* d_z_out, void* d_scratch, int32_t max_n) {
    METRO_CHECK_ARG(plan != nullptr, "metro_plan_bind_heatmaps: plan is NULL");
    if (d_xy_out == nullptr && d_z_out == nullptr && d_scratch == nullptr && max_n == 0) {       // unbind
        plan->heat.xy = plan->heat.z = nullptr; plan->heat.scratch = nullptr; plan->heat.max_n = 0;
        return METRO_OK;
    }
    METRO_CHECK_ARG(d_xy_out != nullptr && d_z_out != nullptr && d_scratch != nullptr,
                    "metro_plan_bind_heatmaps: xy_out, z_out and the scratch go together (all three, or all NULL with max_n 0 to unbind)");
    METRO_CHECK_ARG(max_n >= 1 && max_n <= plan->max_batch, "metro_plan_bind_heatmaps: max_n %d outside [1, %d]", max_n, plan->max_batch);
    METRO_CHECK_ARG(((uintptr_t)d_scratch & 15) == 0 && ((uintptr_t)d_xy_out & 3) == 0 && ((uintptr_t)d_z_out & 3) == 0,
                    "metro_plan_bind_heatmaps: the scratch must be 16-byte aligned, the outputs 4-byte aligned");
    plan->heat.xy = d_xy_out; plan->heat.z = d_z_out; plan->heat.scratch = d_scratch; plan->heat.max_n = max_n;
    return METRO_OK;
}

int64_t metro_plan_modes_scratch_bytes(const MetroPlan* plan, int32_t max_n) {
    if (plan == nullptr || max_n < 1 || max_n > plan->max_batch) return -1;
    return heat_modes_scratch_bytes(max_n, plan->spec.proc_side / plan->spec.stride, plan->spec.n_joints_head, plan->spec.depth,
                                    plan->head_fused);
}

int metro_plan_bind_modes(MetroPlan* plan, int32_t* d_voxel_out, float* d_stats_out, void* d_scratch, int32_t max_n, int32_t k,
                          int32_t radius) {
    METRO_CHECK_ARG(plan != nullptr, "metro_plan_bind_modes: plan is NULL");
    if (d_voxel_out == nullptr && d_stats_out == nullptr && d_scratch == nullptr && max_n == 0 && k == 0 && radius == 0) {      // unbind
        plan->modes.voxel = nullptr; plan->modes.stats = nullptr; plan->modes.scratch = nullptr;
        plan->modes.max_n = plan->modes.k = plan->modes.radius = 0;
        return METRO_OK;
    }
    METRO_CHECK_ARG(d_voxel_out != nullptr && d_stats_out != nullptr && d_scratch != nullptr,
                    "metro_plan_bind_modes: voxel_out, stats_out and the scratch go together (all three, or all NULL with max_n, k and "
                    "radius 0 to unbind)");
    METRO_CHECK_ARG(max_n >= 1 && max_n <= plan->max_batch, "metro_plan_bind_modes: max_n %d outside [1, %d]", max_n, plan->max_batch);
    METRO_CHECK_ARG(k >= 1 && k <= METRO_MAX_MODES, "metro_plan_bind_modes: k %d outside [1, %d]", k, METRO_MAX_MODES);
    METRO_CHECK_ARG(radius >= 0 && radius <= METRO_MAX_MODE_RADIUS, "metro_plan_bind_modes: radius %d outside [0, %d]", radius,
                    METRO_MAX_MODE_RADIUS);
    METRO_CHECK_ARG(((uintptr_t)d_scratch & 15) == 0 && ((uintptr_t)d_voxel_out & 3) == 0 && ((uintptr_t)d_stats_out & 3) == 0,
                    "metro_plan_bind_modes: the scratch must be 16-byte aligned, the outputs 4-byte aligned");
    plan->modes.voxel = d_voxel_out; plan->modes.stats = d_stats_out; plan->modes.scratch = d_scratch;
    plan->modes.max_n = max_n; plan->modes.k = k; plan->modes.radius = radius;
    return METRO_OK;
}

int64_t metro_plan_prior_scratch_bytes(const MetroPlan* plan, int32_t max_n) {
    if (plan == nullptr || max_n < 1 || max_n > plan->max_batch) return -1;
    return heat_posterior_scratch_bytes(max_n, plan->spec.proc_side / plan->spec.stride, plan->spec.n_joints_head, plan->spec.depth,
                                        plan->head_fused);
}

int metro_plan_bind_prior(MetroPlan* plan, const float* d_prior, float* d_post_out, void* d_scratch, int32_t max_n) {
    METRO_CHECK_ARG(plan != nullptr, "metro_plan_bind_prior: plan is NULL");
    if (d_prior == nullptr && d_post_out == nullptr && d_scratch == nullptr && max_n == 0) {       // unbind
        plan->prior.prior = nullptr; plan->prior.post = nullptr; plan->prior.scratch = nullptr; plan->prior.max_n = 0;
        return METRO_OK;
    }
    METRO_CHECK_ARG(plan->track.scratch == nullptr, "metro_plan_bind_prior: a track table is bound (metro_plan_bind_track_prior): one prior per forward");
    METRO_CHECK_ARG(d_prior != nullptr && d_post_out != nullptr && d_scratch != nullptr,
                    "metro_plan_bind_prior: prior, post_out and the scratch go together (all three, or all NULL with max_n 0 to unbind)");
    METRO_CHECK_ARG(max_n >= 1 && max_n <= plan->max_batch, "metro_plan_bind_prior: max_n %d outside [1, %d]", max_n, plan->max_batch);
    METRO_CHECK_ARG(((uintptr_t)d_scratch & 15) == 0 && ((uintptr_t)d_prior & 3) == 0 && ((uintptr_t)d_post_out & 3) == 0,
                    "metro_plan_bind_prior: the scratch must be 16-byte aligned, the prior and the output 4-byte aligned");
    plan->prior.prior = d_prior; plan->prior.post = d_post_out; plan->prior.scratch = d_scratch; plan->prior.max_n = max_n;
    return METRO_OK;
}

int metro_plan_bind_track_prior(MetroPlan* plan, const double* d_state, int32_t capacity, const int32_t* d_slot, const double* d_times,
                                const MetroPlacement* d_records, const int32_t* d_mirror, const MetroTrackPrior* params, float* d_prior_out,
                                int32_t* d_reason_out, float* d_post_out, void* d_scratch, int32_t max_n) {
    METRO_CHECK_ARG(plan != nullptr, "metro_plan_bind_track_prior: plan is NULL");
    if (!d_state && !d_slot && !d_times && !d_records && !d_mirror && !d_prior_out && !d_reason_out && !d_post_out && !d_scratch &&
        capacity == 0 && max_n == 0) {                                                                // unbind
        plan->track = {};
        return METRO_OK;
    }
    METRO_CHECK_ARG(plan->prior.scratch == nullptr, "metro_plan_bind_track_prior: prior rows are bound (metro_plan_bind_prior): one prior per forward");
    METRO_CHECK_ARG(d_state && d_slot && d_times && d_records && d_mirror && params && d_prior_out && d_reason_out && d_post_out && d_scratch,
                    "metro_plan_bind_track_prior: the state, slots, times, records, mirror table, parameters, the three outputs and the "
                    "scratch go together (all of them, or all NULL with capacity and max_n 0 to unbind)");
    METRO_CHECK_ARG(max_n >= 1 && max_n <= plan->max_batch, "metro_plan_bind_track_prior: max_n %d outside [1, %d]", max_n, plan->max_batch);
    METRO_CHECK_ARG(capacity >= 1 && capacity <= METRO_ASSOC_MAX, "metro_plan_bind_track_prior: capacity %d outside [1, %d]", capacity,
                    METRO_ASSOC_MAX);
    METRO_CHECK_ARG(((uintptr_t)d_scratch & 15) == 0 && ((uintptr_t)d_state & 7) == 0 && ((uintptr_t)d_times & 7) == 0 &&
                        ((uintptr_t)d_slot & 3) == 0 && ((uintptr_t)d_records & 3) == 0 && ((uintptr_t)d_mirror & 3) == 0 &&
                        ((uintptr_t)d_prior_out & 3) == 0 && ((uintptr_t)d_reason_out & 3) == 0 && ((uintptr_t)d_post_out & 3) == 0,
                    "metro_plan_bind_track_prior: the scratch must be 16-byte aligned, the state and the times 8-byte, the others 4-byte");
    METRO_CHECK_ARG(params->coords == METRO_COORDS_CAMERA || params->coords == METRO_COORDS_WORLD,
                    "metro_plan_bind_track_prior: coords must be METRO_COORDS_CAMERA or METRO_COORDS_WORLD (got %d)", params->coords);
    METRO_CHECK_ARG(params->depth == METRO_TRACK_PRIOR_DEPTH_NONE || params->depth == METRO_TRACK_PRIOR_DEPTH_ROOT,
                    "metro_plan_bind_track_prior: depth must be METRO_TRACK_PRIOR_DEPTH_NONE or _ROOT (got %d)", params->depth);
    const double values[5] = {params->accel_psd, params->max_age_s, params->near_mm, params->sigma_floor_mm, params->cov_scale};
    static const char* const names[5] = {"accel_psd", "max_age_s", "near_mm", "sigma_floor_mm", "cov_scale"};
    for (int i = 0; i < 5; ++i)
        METRO_CHECK_ARG(__builtin_isfinite(values[i]) && values[i] >= 0.0, "metro_plan_bind_track_prior: %s must be finite and >= 0 (got %g)",
                        names[i], values[i]);
    METRO_CHECK_ARG(params->depth != METRO_TRACK_PRIOR_DEPTH_ROOT || track_prior_root_out(plan->spec) >= 0,
                    "metro_plan_bind_track_prior: METRO_TRACK_PRIOR_DEPTH_ROOT needs the root (head joint %d) in the output order",
                    plan->spec.n_joints_head - 1);
    plan->track.state = d_state; plan->track.slot = d_slot; plan->track.times = d_times; plan->track.records = d_records;
    plan->track.mirror = d_mirror; plan->track.prior = d_prior_out; plan->track.reason = d_reason_out; plan->track.post = d_post_out;
    plan->track.scratch = d_scratch; plan->track.capacity = capacity; plan->track.max_n = max_n; plan->track.params = *params;
    return METRO_OK;
}

int metro_plan_bind_view_fusion(MetroPlan* plan, const float* d_xy, const MetroPlacement* d_records, const int32_t* d_rows, int32_t n_rows,
                                const int32_t* d_starts, int32_t n_persons, const int32_t* d_mirror, const float* d_centres,
                                const MetroViewFusion* params, float* d_points_out, float* d_cov_out, float* d_stats_out,
                                int32_t* d_info_out, float* d_centres_out, int32_t max_n) {
    METRO_CHECK_ARG(plan != nullptr, "metro_plan_bind_view_fusion: plan is NULL");
    if (!d_xy && !d_records && !d_rows && !d_starts && !d_mirror && !d_centres && !params && !d_points_out && !d_cov_out && !d_stats_out &&
        !d_info_out && !d_centres_out && n_rows == 0 && n_persons == 0 && max_n == 0) {               // unbind
        plan->fusion = {};
        return METRO_OK;
    }
    METRO_CHECK_ARG(d_xy && d_records && d_rows && d_starts && d_mirror && params && d_points_out && d_cov_out && d_stats_out && d_info_out &&
                        d_centres_out,
                    "metro_plan_bind_view_fusion: the marginals, records, rows, starts, mirror table, parameters and the five outputs go "
                    "together (all of them, or all NULL with n_rows, n_persons and max_n 0 to unbind); only d_centres may be NULL");
    METRO_CHECK_ARG(max_n >= 1 && max_n <= plan->max_batch, "metro_plan_bind_view_fusion: max_n %d outside [1, %d]", max_n, plan->max_batch);
    METRO_CHECK_ARG(n_rows >= 0 && n_persons >= 0, "metro_plan_bind_view_fusion: negative size (n_rows %d, n_persons %d)", n_rows, n_persons);
    METRO_CHECK_ARG((int64_t)n_persons * plan->spec.n_joints_out <= (int64_t)0x7fffffff / 9,
                    "metro_plan_bind_view_fusion: n_persons %d overflows int32", n_persons);
    METRO_CHECK_ARG((((uintptr_t)d_xy | (uintptr_t)d_records | (uintptr_t)d_rows | (uintptr_t)d_starts | (uintptr_t)d_mirror |
                      (uintptr_t)d_centres | (uintptr_t)d_points_out | (uintptr_t)d_cov_out | (uintptr_t)d_stats_out | (uintptr_t)d_info_out |
                      (uintptr_t)d_centres_out) & 3) == 0,
                    "metro_plan_bind_view_fusion: every pointer must be 4-byte aligned");
    METRO_CHECK_ARG(params->grid >= 2 && params->grid <= 16, "metro_plan_bind_view_fusion: grid %d outside [2, 16]", params->grid);
    METRO_CHECK_ARG(params->n_views >= 1, "metro_plan_bind_view_fusion: n_views must be >= 1 (got %d)", params->n_views);
    METRO_CHECK_ARG(params->weights == METRO_TRI_UNIFORM || params->weights == METRO_TRI_COVARIANCE,
                    "metro_plan_bind_view_fusion: weights must be METRO_TRI_UNIFORM or METRO_TRI_COVARIANCE (got %d)", params->weights);
    METRO_CHECK_ARG(__builtin_isfinite(params->extent_mm) && params->extent_mm > 0.0,
                    "metro_plan_bind_view_fusion: extent_mm must be finite and > 0 (got %g)", params->extent_mm);
    METRO_CHECK_ARG(params->floor > 0.0 && params->floor < 1.0, "metro_plan_bind_view_fusion: floor must lie in (0, 1) (got %g)", params->floor);
    METRO_CHECK_ARG(__builtin_isfinite(params->near_mm) && params->near_mm >= 0.0,
                    "metro_plan_bind_view_fusion: near_mm must be finite and >= 0 (got %g)", params->near_mm);
    METRO_CHECK_ARG(__builtin_isfinite(params->min_det), "metro_plan_bind_view_fusion: min_det must be finite (got %g)", params->min_det);
    METRO_CHECK_ARG(plan->spec.stride > 0 && plan->spec.proc_side / plan->spec.stride >= 2,
                    "metro_plan_bind_view_fusion: the heat-map side must be at least 2 (a bilinear value needs four cells)");
    plan->fusion.xy = d_xy; plan->fusion.records = d_records; plan->fusion.rows = d_rows; plan->fusion.starts = d_starts;
    plan->fusion.mirror = d_mirror; plan->fusion.centres = d_centres; plan->fusion.points = d_points_out; plan->fusion.cov = d_cov_out;
    plan->fusion.stats = d_stats_out; plan->fusion.info = d_info_out; plan->fusion.centres_out = d_centres_out;
    plan->fusion.n_rows = n_rows; plan->fusion.n_persons = n_persons; plan->fusion.max_n = max_n; plan->fusion.params = *params;
    return METRO_OK;
}

int metro_plan_bind_skeleton_modes(MetroPlan* plan, const int32_t* d_voxel, const float* d_stats, int32_t k, const double* d_lengths,
                                   const int32_t* h_edges, int32_t n_edges, const MetroSkeletonModes* params, float* d_prob_out,
                                   int32_t* d_choice_out, float* d_info_out, float* d_coords01_sel_out, int32_t max_n) {
    METRO_CHECK_ARG(plan != nullptr, "metro_plan_bind_skeleton_modes: plan is NULL");
    if (!d_voxel && !d_stats && !d_lengths && !h_edges && !params && !d_prob_out && !d_choice_out && !d_info_out && !d_coords01_sel_out &&
        k == 0 && n_edges == 0 && max_n == 0) {                                                       // unbind
        plan->skel = {};
        return METRO_OK;
    }
    METRO_CHECK_ARG(d_voxel && d_stats && d_lengths && params && d_prob_out && d_choice_out && d_info_out,
                    "metro_plan_bind_skeleton_modes: the modes' voxel and stats, the lengths, the parameters and the three outputs go "
                    "together (all of them, or all NULL with k, n_edges and max_n 0 to unbind); only d_coords01_sel_out may be NULL");
    METRO_CHECK_ARG(max_n >= 1 && max_n <= plan->max_batch, "metro_plan_bind_skeleton_modes: max_n %d outside [1, %d]", max_n, plan->max_batch);
    METRO_CHECK_ARG(k >= 1 && k <= METRO_MAX_MODES, "metro_plan_bind_skeleton_modes: k %d outside [1, %d]", k, METRO_MAX_MODES);
    METRO_CHECK_ARG(n_edges >= 0 && n_edges <= 63, "metro_plan_bind_skeleton_modes: n_edges %d outside [0, 63]", n_edges);
    METRO_CHECK_ARG(n_edges == 0 || h_edges != nullptr, "metro_plan_bind_skeleton_modes: h_edges is NULL with n_edges %d", n_edges);
    METRO_CHECK_ARG(((uintptr_t)d_lengths & 7) == 0 &&
                        (((uintptr_t)d_voxel | (uintptr_t)d_stats | (uintptr_t)d_prob_out | (uintptr_t)d_choice_out | (uintptr_t)d_info_out |
                          (uintptr_t)d_coords01_sel_out) & 3) == 0,
                    "metro_plan_bind_skeleton_modes: the lengths must be 8-byte aligned, the other pointers 4-byte aligned");
    METRO_CHECK_ARG(plan->spec.n_joints_out >= 1 && plan->spec.n_joints_out <= METRO_MAX_JOINTS,
                    "metro_plan_bind_skeleton_modes: %d output joints outside [1, %d]", plan->spec.n_joints_out, METRO_MAX_JOINTS);
    signed char parent[METRO_MAX_JOINTS] = {}, parent_edge[METRO_MAX_JOINTS] = {};
    const char* why = "";
    const int bad = skeleton_schedule(h_edges, n_edges, plan->spec.n_joints_out, parent, parent_edge, &why);
    METRO_CHECK_ARG(bad < 0, "metro_plan_bind_skeleton_modes: edge %d (%d, %d) %s; the plan has %d output joints", bad, h_edges[2 * bad],
                    h_edges[2 * bad + 1], why, plan->spec.n_joints_out);
    for (int i = 0; i < 3; ++i)
        METRO_CHECK_ARG(__builtin_isfinite(params->scale_mm[i]) && params->scale_mm[i] > 0.0,
                        "metro_plan_bind_skeleton_modes: scale_mm[%d] must be finite and > 0 (got %g)", i, params->scale_mm[i]);
    METRO_CHECK_ARG(__builtin_isfinite(params->sigma_mm) && params->sigma_mm > 0.0,
                    "metro_plan_bind_skeleton_modes: sigma_mm must be finite and > 0 (got %g)", params->sigma_mm);
    const double values[3] = {params->sigma_rel, params->cov_scale, params->min_length_mm};
    static const char* const names[3] = {"sigma_rel", "cov_scale", "min_length_mm"};
    for (int i = 0; i < 3; ++i)
        METRO_CHECK_ARG(__builtin_isfinite(values[i]) && values[i] >= 0.0, "metro_plan_bind_skeleton_modes: %s must be finite and >= 0 (got %g)",
                        names[i], values[i]);
    plan->skel = {};
    plan->skel.voxel = d_voxel; plan->skel.stats = d_stats; plan->skel.lengths = d_lengths; plan->skel.prob = d_prob_out;
    plan->skel.choice = d_choice_out; plan->skel.info = d_info_out; plan->skel.coords01_sel = d_coords01_sel_out;
    plan->skel.k = k; plan->skel.n_edges = n_edges; plan->skel.max_n = max_n; plan->skel.params = *params;
    if (n_edges > 0) memcpy(plan->skel.edges, h_edges, sizeof(int32_t) * 2 * (size_t)n_edges);
    memcpy(plan->skel.parent, parent, sizeof(parent)); memcpy(plan->skel.parent_edge, parent_edge, sizeof(parent_edge));
    return METRO_OK;
}

int metro_plan_set_graph_max_batch(MetroPlan* plan, int32_t max_batch_for_graphs) {
    METRO_CHECK_ARG(plan != nullptr && max_batch_for_graphs >= 0, "metro_plan_set_graph_max_batch: bad argument");
    plan->graph_max_batch = max_batch_for_graphs;
    return METRO_OK;
}

static int forward_impl(MetroPlan* plan, const float* d_images_nhwc, int32_t n, float* d_poses_out, float* d_coords01,
                        void* d_workspace, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // heat-map, mode, prior, track-prior, view-fusion or skeleton buffers bound: plain launches, the captured forwards do not write them
    if (plan == nullptr || n > plan->graph_max_batch || n < 1 || plan->heat.scratch != nullptr || plan->modes.scratch != nullptr ||
        plan->prior.scratch != nullptr || plan->track.scratch != nullptr || plan->fusion.points != nullptr || plan->skel.prob != nullptr)
        return run_layers(plan, d_images_nhwc, n, d_poses_out, d_workspace, stream, -1, nullptr, d_coords01);
    // small batches are launch-latency bound (57 dependent launches): replay a captured hipGraph
    GraphEntry* hit = nullptr;
    for (GraphEntry& g : plan->graphs)
        if (g.n == n && g.images == d_images_nhwc && g.poses == d_poses_out && g.coords01 == d_coords01 && g.ws == d_workspace)
            hit = &g;
    if (hit == nullptr) {
        if (plan->graphs.size() >= 16) {            // bounded cache: drop the oldest capture
            if (plan->graphs.front().exec) (void)hipGraphExecDestroy(plan->graphs.front().exec);
            plan->graphs.erase(plan->graphs.begin());
        }
        plan->graphs.push_back(GraphEntry{n, d_images_nhwc, d_poses_out, d_coords01, d_workspace, stream, nullptr, 0});
        hit = &plan->graphs.back();
    }
    if (hit->exec == nullptr) {
        if (hit->eager_runs == 0) {                  // first sight of this key: plain launches (sets kernel attributes)
            hit->eager_runs = 1;
            return run_layers(plan, d_images_nhwc, n, d_poses_out, d_workspace, stream, -1, nullptr, d_coords01);
        }
        hipGraph_t graph = nullptr;
        if (plan->cap_stream == nullptr) METRO_HIP_CHECK(hipStreamCreateWithFlags(&plan->cap_stream, hipStreamNonBlocking));
        METRO_HIP_CHECK(hipStreamBeginCapture(plan->cap_stream, hipStreamCaptureModeThreadLocal));
        const int st = run_layers(plan, d_images_nhwc, n, d_poses_out, d_workspace, plan->cap_stream, -1, nullptr, d_coords01);
        const hipError_t e = hipStreamEndCapture(plan->cap_stream, &graph);
        if (st != METRO_OK) { if (graph) (void)hipGraphDestroy(graph); return st; }
        if (e != hipSuccess) { set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return METRO_ERR_HIP; }
        const hipError_t ei = hipGraphInstantiate(&hit->exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ei != hipSuccess) { hit->exec = nullptr; set_error("hipGraphInstantiate: %s", hipGetErrorString(ei)); return METRO_ERR_HIP; }
    }
    METRO_HIP_CHECK(hipGraphLaunch(hit->exec, stream));
    return METRO_OK;
}

int metro_forward(MetroPlan* plan, const float* d_images_nhwc, int32_t n, float* d_poses_out,
                  void* d_workspace, void* stream) {
    return forward_impl(plan, d_images_nhwc, n, d_poses_out, nullptr, d_workspace, stream);
}

int metro_forward_coords01(MetroPlan* plan, const float* d_images_nhwc, int32_t n, float* d_poses_out,
                           float* d_coords01_out, void* d_workspace, void* stream) {
    METRO_CHECK_ARG(d_coords01_out != nullptr && d_poses_out != nullptr, "metro_forward_coords01: NULL poses / coords01 pointer");
    return forward_impl(plan, d_images_nhwc, n, d_poses_out, d_coords01_out, d_workspace, stream);
}

int metro_forward_u8(MetroPlan* plan, const uint8_t* d_images_nhwc, int32_t n, float* d_poses_out, float* d_coords01_out,
                     void* d_workspace, void* stream) {
    METRO_CHECK_ARG(plan != nullptr, "metro_forward_u8: plan is NULL");
    METRO_CHECK_ARG(plan->spec.precision == METRO_PREC_F16,
                    "metro_forward_u8: uint8 crops run on f16 plans only; for this precision expand them with metro_images_u8_to_f32 "
                    "and call metro_forward");
    METRO_CHECK_ARG(d_poses_out != nullptr, "metro_forward_u8: NULL poses pointer");
    METRO_CHECK_ARG(((uintptr_t)d_images_nhwc & 15) == 0, "metro_forward_u8: uint8 crops must start at a 16-byte aligned address (got %p)",
                    (const void*)d_images_nhwc);
    // eager: the captured-forward cache is keyed for metro_forward's fp32 images only
    return run_layers(plan, reinterpret_cast<const float*>(d_images_nhwc), n, d_poses_out, d_workspace, static_cast<hipStream_t>(stream), -1,
                      nullptr, d_coords01_out, true);
}

int64_t metro_moments_scratch_bytes(const MetroSpec* spec, int32_t n) {
    if (spec == nullptr || n <= 0 || spec->stride <= 0 || spec->proc_side / spec->stride < 2 || spec->n_joints_head <= 0) return -1;
    return moments_scratch_bytes(n, spec->proc_side / spec->stride, spec->n_joints_head);
}

int metro_forward_moments(MetroPlan* plan, const void* d_images_nhwc, int32_t images_u8, int32_t n, float* d_poses_out,
                          float* d_coords01_out, float* d_cov01_out, float* d_peak_out, void* d_moments_scratch,
                          void* d_workspace, void* stream) {
    METRO_CHECK_ARG(plan != nullptr, "metro_forward_moments: plan is NULL");
    METRO_CHECK_ARG(d_poses_out != nullptr, "metro_forward_moments: NULL poses pointer");
    METRO_CHECK_ARG(images_u8 == 0 || images_u8 == 1, "metro_forward_moments: images_u8 must be 0 or 1 (got %d)", images_u8);
    METRO_CHECK_ARG(!images_u8 || plan->spec.precision == METRO_PREC_F16,
                    "metro_forward_moments: uint8 crops run on f16 plans only; for this precision expand them with "
                    "metro_images_u8_to_f32");
    METRO_CHECK_ARG(!images_u8 || ((uintptr_t)d_images_nhwc & 15) == 0,
                    "metro_forward_moments: uint8 crops must start at a 16-byte aligned address (got %p)", d_images_nhwc);
    METRO_CHECK_ARG((d_cov01_out != nullptr) == (d_peak_out != nullptr) && (d_cov01_out != nullptr) == (d_moments_scratch != nullptr),
                    "metro_forward_moments: cov01_out, peak_out and the moments scratch go together (all three or none)");
    METRO_CHECK_ARG(((uintptr_t)d_moments_scratch & 15) == 0, "metro_forward_moments: the moments scratch must be 16-byte aligned");
    MomentsOut mo;
    mo.scratch = d_moments_scratch; mo.cov01 = d_cov01_out; mo.peak = d_peak_out;
    // eager, like metro_forward_u8: the captured-forward cache is keyed for metro_forward / metro_forward_coords01 only
    return run_layers(plan, static_cast<const float*>(d_images_nhwc), n, d_poses_out, d_workspace, static_cast<hipStream_t>(stream), -1,
                      nullptr, d_coords01_out, images_u8 != 0, mo);
}

int metro_forward_status(const MetroPlan* plan, const void* d_workspace, int32_t n, void* stream_, int32_t* n_nonfinite_out) {
    METRO_CHECK_ARG(plan && d_workspace && n_nonfinite_out, "metro_forward_status: NULL argument");
    METRO_CHECK_ARG(n > 0 && n <= plan->max_batch, "metro_forward_status: batch %d outside [1, %d]", n, plan->max_batch);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    std::vector<int32_t> host((size_t)n);
    METRO_HIP_CHECK(hipMemcpyAsync(host.data(), static_cast<const char*>(d_workspace) + plan->slot_offset[S_STATUS], (size_t)n * 4,
                                   hipMemcpyDeviceToHost, stream));
    METRO_HIP_CHECK(hipStreamSynchronize(stream));
    int32_t bad = 0;
    for (int32_t v : host) bad += v != 0;
    *n_nonfinite_out = bad;
    if (bad) {
        set_error("%d of %d crops reached the soft-argmax with non-finite statistics%s", bad, n,
                  plan->spec.precision == METRO_PREC_F16 ? " (fp16 storage overflows at 65504: run this model with precision f32m or f64)" : "");
        return METRO_ERR_NONFINITE;
    }
    return METRO_OK;
}


int metro_forward_upto(MetroPlan* plan, const float* d_images_nhwc, int32_t n, float* d_poses_out,
                       void* d_workspace, void* stream, int32_t last_layer) {
    return run_layers(plan, d_images_nhwc, n, d_poses_out, d_workspace, static_cast<hipStream_t>(stream), last_layer, nullptr);
}

int metro_forward_timed(MetroPlan* plan, const float* d_images_nhwc, int32_t n, float* d_poses_out,
                        void* d_workspace, void* stream, float* ms_out) {
    METRO_CHECK_ARG(ms_out != nullptr, "metro_forward_timed: ms_out is NULL");
    return run_layers(plan, d_images_nhwc, n, d_poses_out, d_workspace, static_cast<hipStream_t>(stream), -1, ms_out);
}

}  // extern "C"
