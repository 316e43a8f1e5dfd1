// Planner of libmetro_hip.so.  metro_plan_create restates, in C++, the graph that the reference builds in Python at export time
// (reference src/main.py:106-128 -> src/model/volumetric.py:152-216 -> src/model/architectures.py:24-35 ->
// src/model/resnet_v2.py:142-312 -> src/model/resnet_utils.py:263-350) as a flat list of kernel launches over a pre-planned
// workspace.  The test-side oracle (oracle/spec.py) restates the same control flow independently in Python;
// tests/test_abi_and_plan.py compares the two layer by layer.
// The bottleneck units are planned in three steps: unit_geometry (what the reference computes), choose_fusion (which launches
// a unit becomes) and emit_unit (layers, slots, parameters).  tests/test_plan_snapshot.py holds the result byte for byte.
#include <algorithm>
#include <cmath>
#include <string>

#include "plan.h"

using namespace metro;

namespace {

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// TF 'SAME' padding: out = ceil(in/s); total = max((out-1)*s + k_eff - in, 0); beg = total/2
int tf_same_pad_beg(int in, int k_eff, int s) {
    const int out = (in + s - 1) / s;
    return std::max((out - 1) * s + k_eff - in, 0) / 2;
}

int stem_side(int proc_side) { return (proc_side + 6 - 7) / 2 + 1; }   // conv1 7x7/2, explicit pad 3: 128
int pool_side(int s2) { return (s2 + 2 - 3) / 2 + 1; }                 // pool1 3x3/2, zero pad 1: 64

// ---- step 1: geometry ----------------------------------------------------------------------------------------------------------
// One bottleneck unit as the reference computes it; nothing about launches, slots or precision.
struct UnitGeom {
    int block, unit, n_units;         // 1-based block and unit, units in the block
    int c_in, width, c_out;           // unit input channels, bottleneck width, 4 x width
    int side_in, side_out, stride, rate;   // stride and rate of conv2 (the stride: also of the shortcut's sub-sampling)
    bool centered, project;           // centred stride; projection shortcut (resnet_v2.py:120-125)
    int shift;                        // first input pixel of the strided shortcut (resnet_v2.py:113-115)
    int pad_beg;                      // conv2's leading pad (conv2d_same, resnet_utils.py:82-135)
    std::string name, scope;          // "block1/unit_1", "block1/unit_1/bottleneck_v2"
};

// The reference's block table (resnet_v2.py:272-312) run through stack_blocks_dense (resnet_utils.py:307-348): the C++ twin of
// oracle/spec.py: schedule.
int unit_geometry(const MetroSpec& sp, std::vector<UnitGeom>* units) {
    bool centered[3] = {false, false, false};
    if (sp.centered_stride) {
        int i_last = sp.arch == 50 ? (int)std::lround(std::log2((double)sp.stride)) - 3    // :279-281
                                   : (int)std::log2((double)sp.stride) - 3;                // :301-302
        if (sp.arch != 50 && i_last < 0) i_last += 3;   // Python c[-1]
        if (i_last >= 0 && i_last < 3) centered[i_last] = true;
    }
    const int n_units[4] = {3, 4, sp.arch == 50 ? 6 : 23, 3};
    const int block_stride[4] = {2, 2, 2, 1};
    const double output_stride = sp.stride / 4.0;    // resnet_v2.py:215 (float division)
    int current_stride = 1, rate = 1;
    int side = pool_side(stem_side(sp.proc_side)), c = sp.base_width;
    for (int b = 0; b < 4; ++b) {
        for (int u = 1; u <= n_units[b]; ++u) {
            UnitGeom g;
            g.block = b + 1; g.unit = u; g.n_units = n_units[b];
            const int unit_stride = u == n_units[b] ? block_stride[b] : 1;   // resnet_v2.py:260-269
            g.centered = u == n_units[b] && b < 3 && centered[b];
            if ((double)current_stride == output_stride) {
                g.stride = 1; g.rate = rate; rate *= unit_stride;            // :325-327
            } else {
                g.stride = unit_stride; g.rate = 1; current_stride *= unit_stride;   // :329-333
                if ((double)current_stride > output_stride) { set_error("The target output_stride cannot be reached."); return METRO_ERR_INVALID_ARG; }
            }
            g.c_in = c; g.width = sp.base_width << b; g.c_out = 4 * g.width;
            g.side_in = side; g.side_out = g.stride == 2 ? (side + 1) / 2 : side;
            g.shift = (g.centered && g.stride == 2) ? 1 : 0;
            g.project = g.c_in != g.c_out;
            const int k_eff = 3 + 2 * (g.rate - 1);
            g.pad_beg = (g.stride == 1 || g.centered) ? tf_same_pad_beg(side, k_eff, g.stride) : (k_eff - 1) / 2;
            g.name = "block" + std::to_string(g.block) + "/unit_" + std::to_string(u);
            g.scope = g.name + "/bottleneck_v2";
            units->push_back(g);
            side = g.side_out; c = g.c_out;
        }
    }
    if ((double)current_stride != output_stride) { set_error("The target output_stride cannot be reached."); return METRO_ERR_INVALID_ARG; }
    if (side != sp.proc_side / sp.stride) { set_error("internal: output side %d != %d", side, sp.proc_side / sp.stride); return METRO_ERR_STATE; }
    return METRO_OK;
}

// ---- step 2: fusion choice -----------------------------------------------------------------------------------------------------
// Which launches a unit becomes.  The plain unit is [shortcut] conv1 conv2 conv3(+shortcut): four launches, all tensors in HBM.
enum class Conv1At { OwnLaunch, Pair, FrontOfConv2, PrevConv3 };     // Pair: one launch with the projection shortcut
enum class ShortcutFrom { Identity, OwnLaunch, Pair, InConv3, RebuiltInConv3, Compact };
enum class SumTo { Stored, OnChip, SubSampled };
struct UnitFusion {
    Conv1At conv1 = Conv1At::OwnLaunch;
    ShortcutFrom shortcut = ShortcutFrom::Identity;
    SumTo sum = SumTo::Stored;            // what becomes of the unit's output x_u = conv3 + shortcut
    int sub_off = 0, sub_side = 0;        // SubSampled: pixels (sub_off + 2 i, sub_off + 2 j), sub_side of them a side
    bool carries_next_conv1 = false;      // the conv3 launch also runs conv1 of the next unit on its output tile
};

// A batch-1 fp16 stride-1 SAME k x k convolution on a side x side map: what the kernel predicates are asked about a layer.
// The choice must hold for EVERY batch the plan may run (the layer list is fixed): probed at n = 1.
MetroConvDesc probe_desc(int side, int c_in, int c_out, int k, bool prologue, bool relu) {
    MetroConvDesc d{};
    d.n = 1; d.h_in = d.w_in = d.h_out = d.w_out = side; d.c_in = d.in_pix_stride = c_in; d.c_out = c_out;
    d.kh = d.kw = k; d.stride = 1; d.dilation = 1; d.pad_top = d.pad_left = k / 2;
    d.has_prologue = prologue; d.relu = relu; d.res_stride = 1;
    d.out_dtype = d.in_dtype = METRO_F16;
    return d;
}

// a fused form with the shape of its parts only (no tensors): probes of conv_form_supported / conv_pw64_supported
ConvFused form_probe(ConvForm form, int c2) {
    ConvFused f;
    f.form = form; f.next.c2 = c2;
    return f;
}

int choose_fusion(const std::vector<UnitGeom>& G, bool fast, std::vector<UnitFusion>* fusions) {
    std::vector<UnitFusion>& F = *fusions;
    F.assign(G.size(), UnitFusion{});
    for (size_t i = 0; i < G.size(); ++i) {
        const UnitGeom& g = G[i];
        UnitFusion& f = F[i];
        const bool last = g.unit == g.n_units;      // units i - 1 / i + 1 below are in g's block whenever they are looked at
        const bool conv1_done = i > 0 && F[i - 1].carries_next_conv1;
        const bool prev_on_chip = i > 0 && F[i - 1].sum == SumTo::OnChip;
        const bool proj_s1 = fast && g.project && g.stride == 1;
        const bool b1_shape = g.c_in == 64 && g.width == 64 && g.c_out == 256;      // block1/unit_1 of the 64-wide nets
        // block1/unit_1 (64-channel input): conv1 in front of conv2 inside the weight-resident 3x3 kernel, the projection
        // shortcut inside the conv3 (+ next conv1) launch: two launches, no shortcut / t1 tensors
        const MetroConvDesc conv3 = probe_desc(g.side_in, 64, 256, 1, false, false);
        const bool unit_fused = proj_s1 && b1_shape && g.rate == 1 && !last && !conv1_done && tuning_knob("METRO_UNIT1_FUSED", 1) &&
                                conv3x3_c64_supported(probe_desc(g.side_in, 64, 64, 3, false, true)) &&
                                conv_form_supported(conv3, form_probe(ConvForm::NextProj, g.width));
        // ... and none of the block's 256-channel sums in HBM (conv_pw64 REB / OUTM), in a block of three units: x_1 stays on
        // chip (it only feeds unit 2's conv1, inside unit 1's conv3 launch), so unit 2 has no residual tensor to read -- its
        // conv3 launch rebuilds its identity shortcut x_1 from unit 1's conv2 output and conv3 / shortcut parameters
        if (unit_fused && g.unit == 1 && g.n_units == 3 && tuning_knob("METRO_B1_REBUILD", 1) &&
            conv_form_supported(conv3, form_probe(ConvForm::NextRebuild, g.width)))
            f.sum = SumTo::OnChip;
        // shortcut + conv1 as one launch.  Measured on MI355X (batch 64): pays when conv1 fills whole 128-cout tiles and the pair is
        // not huge (block2/block3 of ResNet-50/101: -9 / -7 us); block1 (width 64: a half-empty tile in the tiled kernel) pairs only
        // in the persistent kernel.  Block4's pair too (1024 -> 2048 + 512 in one conv_gemm4w launch: the 134 MB input read once,
        // one launch fewer; same-box A/B batch 256 -0.4 %, batch 64 0)
        static const int pair_max_cout = tuning_knob("METRO_PAIR_MAX_COUT", 2048);
        bool pair = proj_s1 && g.c_out % 256 == 0 && g.c_in % 64 == 0 && !unit_fused;
        if (pair && !(g.width % 128 == 0 && g.c_out <= pair_max_cout)) {
            ConvFused pf = form_probe(ConvForm::Pair, 0);
            pf.pair.split = g.c_out; pf.pair.c_out2 = g.width; pf.pair.relu2 = 1;
            pair = b1_shape && conv_pw64_supported(probe_desc(g.side_in, g.c_in, g.c_out + g.width, 1, true, false), pf);
        }
        f.conv1 = unit_fused ? Conv1At::FrontOfConv2 : conv1_done ? Conv1At::PrevConv3 : pair ? Conv1At::Pair : Conv1At::OwnLaunch;
        if (unit_fused) f.shortcut = ShortcutFrom::InConv3;
        else if (prev_on_chip) f.shortcut = ShortcutFrom::RebuiltInConv3;
        else if (g.project) f.shortcut = f.conv1 == Conv1At::Pair ? ShortcutFrom::Pair : ShortcutFrom::OwnLaunch;
        // the previous launch wrote exactly the pixels this unit's sub-sampled shortcut reads, compactly
        else f.shortcut = i > 0 && F[i - 1].sum == SumTo::SubSampled ? ShortcutFrom::Compact : ShortcutFrom::Identity;
        // what the unit after the rebuild reads of this sum: every pixel (it runs at stride 1: stride-4 nets), or every second one
        if (f.shortcut == ShortcutFrom::RebuiltInConv3 && !last && G[i + 1].stride == 2) {
            f.sum = SumTo::SubSampled; f.sub_off = G[i + 1].shift; f.sub_side = G[i + 1].side_out;
        }
        // conv1 of the next unit rides in the conv3 launch.  Width 64 (block1, full 256-channel rows per pixel tile): the ring
        // kernel's fusion (METRO_FUSE2); width 128 (block2, 128 -> 512 on 32-wide maps): the persistent kernel with all 512
        // channels of a pixel tile in one block.  The InConv3 / RebuiltInConv3 launches are fused launches by form
        if (fast && !last && g.stride == 1) {
            MetroConvDesc d = probe_desc(g.side_out, g.width, g.c_out, 1, false, false);      // conv3 + shortcut tensor
            d.has_residual = 1; d.res_h = d.res_w = g.side_out;
            f.carries_next_conv1 = unit_fused || f.shortcut == ShortcutFrom::RebuiltInConv3 ||
                                   (d.c_in == 128 ? conv_form_supported(d, form_probe(ConvForm::Next, g.width))
                                                  : conv_f16_fuse2_supported(d, g.width));
        }
    }
    // a sum that is not stored must be consumed by the next unit's launch, which the kernels run only on a plain unit
    for (size_t i = 1; i < G.size(); ++i) {
        const UnitGeom& g = G[i];
        if (F[i - 1].sum == SumTo::OnChip && !(F[i].shortcut == ShortcutFrom::RebuiltInConv3 && F[i].conv1 == Conv1At::PrevConv3 &&
                                               !g.project && g.stride == 1 && g.rate == 1)) {
            set_error("internal: block1 rebuild chain planned for a unit 2 that is not plain"); return METRO_ERR_STATE;
        }
        if (F[i - 1].sum == SumTo::SubSampled && !(F[i].shortcut == ShortcutFrom::Compact && g.stride == 2)) {
            set_error("internal: compact shortcut planned for a unit that is not strided"); return METRO_ERR_STATE;
        }
    }
    return METRO_OK;
}

// ---- step 3: emission ----------------------------------------------------------------------------------------------------------
struct ParamShape { int c_out, kh = 1, kw = 1, c_in = 1, kw_pad = 1, c_in_pad = 1; };

// One convolution layer; the defaults are the common case (1x1, stride 1, no pad, no ReLU, no residual, activation dtype).
struct ConvSpec {
    std::string name, scope;            // layer name; slim scope below root, e.g. "block1/unit_1/bottleneck_v2/conv1"
    std::string bn_fold, prologue_bn;   // scope of the BN folded into it ("" = own biases); of the pre-activation BN on its input
    int in_slot, out_slot, side_in, c_in, side_out, c_out;
    int k = 1, stride = 1, rate = 1, pad_beg = 0;
    bool relu = false;
    int res_slot = S_NONE, res_side = 0, res_stride = 1, res_offset = 0;
    int out_dtype = -1, in_dtype = -1;  // -1: the activation dtype
};

struct Builder {
    MetroPlan* p;
    std::string root;

    int add_param(const std::string& name, int kind, const std::string& conv_var, const std::string& bn_var, int dtype, ParamShape s) {
        MetroParamInfo pi;
        memset(&pi, 0, sizeof(pi));     // with the padding: metro_plan_param_info copies it out
        snprintf(pi.name, sizeof(pi.name), "%s", name.c_str());
        snprintf(pi.conv_var, sizeof(pi.conv_var), "%s", conv_var.c_str());
        snprintf(pi.bn_var, sizeof(pi.bn_var), "%s", bn_var.c_str());
        pi.kind = kind; pi.dtype = dtype;
        pi.c_out = s.c_out; pi.kh = s.kh; pi.kw = s.kw; pi.c_in = s.c_in; pi.kw_pad = s.kw_pad; pi.c_in_pad = s.c_in_pad;
        const int64_t elems = kind == METRO_PARAM_CONV_W ? (int64_t)s.c_out * s.kh * s.kw_pad * s.c_in_pad : s.c_out;
        pi.bytes = elems * dtype_bytes(dtype); pi.offset = p->param_bytes;
        p->param_bytes = align_up(p->param_bytes + pi.bytes, 256);
        p->params.push_back(pi);
        return (int)p->params.size() - 1;
    }
    int wdt() const { return p->fast ? METRO_F16 : p->spec.precision == METRO_PREC_F32M ? METRO_F32 : METRO_F64; }
    int bdt() const { return p->fast || p->spec.precision == METRO_PREC_F32M ? METRO_F32 : METRO_F64; }

    // The parameter group of one convolution `lname`: W, bias and, with a pre-activation BN on its input, that BN's scale and
    // shift.  `scope` is the conv's slim scope below root, bn_fold the scope of the BN folded into it ("" = own biases).
    ConvParams conv_params(const std::string& lname, const std::string& scope, const std::string& bn_fold,
                           const std::string& prologue_bn, int c_out, int k, int c_in) {
        const std::string conv_var = root + "/" + scope, bn_var = bn_fold.empty() ? "" : root + "/" + bn_fold;
        ConvParams g;
        g.w = add_param(lname + "/W", METRO_PARAM_CONV_W, conv_var, bn_var, wdt(), {c_out, k, k, c_in, k, c_in});
        g.bias = add_param(lname + "/bias", METRO_PARAM_BIAS, conv_var, bn_var, bdt(), {c_out});
        if (!prologue_bn.empty()) {
            g.scale = add_param(lname + "/pro_scale", METRO_PARAM_PRO_SCALE, "", root + "/" + prologue_bn, wdt(), {c_in});
            g.shift = add_param(lname + "/pro_shift", METRO_PARAM_PRO_SHIFT, "", root + "/" + prologue_bn, wdt(), {c_in});
        }
        return g;
    }

    void need(int slot, int64_t bytes) { if (slot >= 0) p->slot_bytes_per_image[slot] = std::max(p->slot_bytes_per_image[slot], bytes); }
    void fill_info(Layer& L, const std::string& lname, double flops) {
        MetroLayerInfo& I = L.info;
        const MetroConvDesc& cd = L.cd;
        snprintf(I.name, sizeof(I.name), "%s", lname.c_str());
        I.kind = L.kind; I.h_in = cd.h_in; I.w_in = cd.w_in; I.c_in = cd.c_in; I.h_out = cd.h_out; I.w_out = cd.w_out; I.c_out = cd.c_out;
        I.kh = cd.kh; I.kw = cd.kw; I.stride = cd.stride; I.dilation = cd.dilation; I.pad_top = cd.pad_top; I.pad_left = cd.pad_left;
        I.has_prologue = cd.has_prologue; I.relu = cd.relu; I.has_residual = cd.has_residual;
        I.res_stride = cd.res_stride; I.res_offset = cd.res_offset; I.out_dtype = cd.out_dtype;
        I.flops_per_image = flops; p->flops_per_image += flops;
    }
    // a further 1x1 convolution (c_out x c_in on a side x side map) computed inside L's launch
    void add_fused_flops(Layer& L, int side, int c_out, int c_in) {
        const double flops = 2.0 * side * side * (double)c_out * c_in;
        L.info.flops_per_image += flops; p->flops_per_image += flops;
    }

    MetroConvDesc conv_desc(const ConvSpec& c) const {
        MetroConvDesc cd{};       // cd.n is filled per call
        cd.h_in = cd.w_in = c.side_in; cd.c_in = c.c_in; cd.in_pix_stride = c.c_in;
        cd.h_out = cd.w_out = c.side_out; cd.c_out = c.c_out;
        cd.kh = cd.kw = c.k; cd.stride = c.stride; cd.dilation = c.rate; cd.pad_top = cd.pad_left = c.pad_beg;
        cd.has_prologue = !c.prologue_bn.empty(); cd.relu = c.relu; cd.has_residual = c.res_slot != S_NONE;
        cd.res_h = cd.res_w = c.res_side; cd.res_stride = c.res_stride; cd.res_offset = c.res_offset;
        cd.out_dtype = c.out_dtype < 0 ? p->act_dtype : c.out_dtype; cd.in_dtype = c.in_dtype < 0 ? p->act_dtype : c.in_dtype;
        return cd;
    }

    Layer conv(const ConvSpec& c) {
        Layer L;
        const MetroConvDesc& cd = L.cd = conv_desc(c);
        L.main = conv_params(c.name, c.scope, c.bn_fold, c.prologue_bn, c.c_out, c.k, c.c_in);
        L.in_slot = c.in_slot; L.out_slot = c.out_slot; L.res_slot = c.res_slot;
        need(c.out_slot, (int64_t)c.side_out * c.side_out * c.c_out * dtype_bytes(cd.out_dtype));
        fill_info(L, c.name, (double)2.0 * c.side_out * c.side_out * c.c_out * c.k * c.k * c.c_in);
        return L;
    }

    // Projection shortcut (c_out outputs, bias, no ReLU) and conv1 (width outputs, folded BN + ReLU) of a unit read the same
    // pre-activated tensor: one launch over concatenated weight rows (reference resnet_v2.py:122-128).  Parameter tensors keep
    // their own names and are laid out back to back so the kernel sees one [c_out + width][c_in] matrix.
    int shortcut_conv1_pair(const UnitGeom& g, int in_slot, Layer* out) {
        Layer& L = *out;
        const int side = g.side_in;
        L.form = LayerForm::Pair;
        L.cd = conv_desc({g.name + "/shortcut+conv1", "", "", g.scope + "/preact", in_slot, S_SC, side, g.c_in, side, g.c_out + g.width});
        const std::string sc = root + "/" + g.scope + "/shortcut", c1 = root + "/" + g.scope + "/conv1", pre = root + "/" + g.scope + "/preact";
        const ParamShape w_sc = {g.c_out, 1, 1, g.c_in, 1, g.c_in}, w_c1 = {g.width, 1, 1, g.c_in, 1, g.c_in};
        L.main.w = add_param(g.name + "/shortcut/W", METRO_PARAM_CONV_W, sc, "", METRO_F16, w_sc);
        L.conv1.w = add_param(g.name + "/conv1/W", METRO_PARAM_CONV_W, c1, c1 + "/BatchNorm", METRO_F16, w_c1);
        L.main.bias = add_param(g.name + "/shortcut/bias", METRO_PARAM_BIAS, sc, "", METRO_F32, {g.c_out});
        L.conv1.bias = add_param(g.name + "/conv1/bias", METRO_PARAM_BIAS, c1, c1 + "/BatchNorm", METRO_F32, {g.width});
        // contiguity (sizes are multiples of the 256-byte blob alignment for c_out % 256 == 0, c_in % 64 == 0)
        if (p->params[L.conv1.w].offset != p->params[L.main.w].offset + p->params[L.main.w].bytes ||
            p->params[L.conv1.bias].offset != p->params[L.main.bias].offset + p->params[L.main.bias].bytes) {
            set_error("internal: fused pair parameters of %s are not contiguous in the blob", g.name.c_str());
            return METRO_ERR_STATE;       // the kernel reads conv1's rows at w + c_out * c_in: never launch on a broken layout
        }
        L.main.scale = add_param(g.name + "/shortcut/pro_scale", METRO_PARAM_PRO_SCALE, "", pre, METRO_F16, {g.c_in});
        L.main.shift = add_param(g.name + "/shortcut/pro_shift", METRO_PARAM_PRO_SHIFT, "", pre, METRO_F16, {g.c_in});
        L.in_slot = in_slot; L.out_slot = S_SC; L.c2 = g.width; L.out2_slot = S_T1;
        need(S_SC, (int64_t)side * side * g.c_out * 2); need(S_T1, (int64_t)side * side * g.width * 2);
        fill_info(L, g.name + "/shortcut+conv1", 2.0 * side * side * (double)(g.c_out + g.width) * g.c_in);
        L.info.c_out = g.c_out;      // the primary output tensor (S_SC) has c_out channels
        return METRO_OK;
    }

    // conv1 of the unit (folded BN + ReLU, on the pre-activated unit input) in FRONT of its conv2 layer L, whose input becomes
    // the unit's raw input in x_slot (reference resnet_v2.py:119,127-132)
    void fuse_conv1_in_front(Layer& L, const UnitGeom& g, int x_slot) {
        L.conv1 = conv_params(g.name + "/conv1", g.scope + "/conv1", g.scope + "/conv1/BatchNorm", g.scope + "/preact", g.width, 1, g.c_in);
        L.form = LayerForm::Conv1Conv2; L.in_slot = x_slot;
        snprintf(L.info.name, sizeof(L.info.name), "%s/conv1+conv2", g.name.c_str());
        L.info.fused_flags |= METRO_FUSED_CONV1_IN_FRONT;
        add_fused_flops(L, g.side_in, g.width, g.c_in);
    }

    // The unit's projection shortcut (bias, on the pre-activated unit input in x_slot) computed inside its conv3 layer L instead
    // of being read from a tensor (reference resnet_v2.py:119,122-125,138)
    void fuse_projection_shortcut(Layer& L, const UnitGeom& g, int x_slot) {
        L.psc = conv_params(g.name + "/shortcut", g.scope + "/shortcut", "", g.scope + "/preact", g.c_out, 1, g.c_in);
        L.form = LayerForm::NextProj; L.psc_slot = x_slot;
        L.info.fused_flags |= METRO_FUSED_PROJECTION_SHORTCUT;
        add_fused_flops(L, g.side_in, g.c_out, g.c_in);
    }

    // conv1 of the NEXT unit `nx` (folded BN + ReLU, pre-activation prologue of that unit) behind the conv3 layer L: a second GEMM on
    // the LDS-resident output tile (reference resnet_v2.py:119,127-128 of unit u+1).  Parameter names stay those of the next unit.
    void fuse_next_conv1(Layer& L, const UnitGeom& nx) {
        L.next = conv_params(nx.name + "/conv1", nx.scope + "/conv1", nx.scope + "/conv1/BatchNorm", nx.scope + "/preact", nx.width, 1, nx.c_in);
        L.c2 = nx.width; L.out2_slot = S_T1;
        if (L.form == LayerForm::Plain) L.form = LayerForm::Next;      // NextProj / NextRebuild: set by the shortcut fusions before
        need(S_T1, (int64_t)nx.side_in * nx.side_in * nx.width * 2);
        const std::string name = std::string(L.info.name) + "+" + nx.name.substr(nx.name.find('/') + 1) + "/conv1";
        snprintf(L.info.name, sizeof(L.info.name), "%s", name.c_str());
        add_fused_flops(L, nx.side_in, nx.width, nx.c_in);
    }

    // The layers of one unit.  *x_slot: in, the slot of the unit's input; out, of its output.
    int prev3 = -1;       // layer index of the previous unit's conv3 launch
    int emit_unit(const UnitGeom& g, const UnitFusion& f, const UnitGeom* next_unit, int* x_slot) {
        const std::string &un = g.name, &sc = g.scope;
        const int x = *x_slot;
        // the rebuilding launch does not read x (= S_X1, which x_1 never reached); S_X0 still holds x_0, which it reads
        const int out = f.shortcut == ShortcutFrom::RebuiltInConv3 ? x : x == S_X0 ? S_X1 : S_X0;
        if (f.conv1 == Conv1At::Pair) {
            Layer L;
            if (const int st = shortcut_conv1_pair(g, x, &L)) return st;
            p->layers.push_back(L);
        } else if (f.conv1 == Conv1At::OwnLaunch) {
            if (f.shortcut == ShortcutFrom::OwnLaunch) {
                // conv1x1(shift(preact), stride s) + bias: input pixel = shift + s*ho
                ConvSpec c{un + "/shortcut", sc + "/shortcut", "", sc + "/preact", x, S_SC, g.side_in, g.c_in, g.side_out, g.c_out};
                c.stride = g.stride; c.pad_beg = -g.shift;
                p->layers.push_back(conv(c));
            }
            // conv1: 1x1 on preact, BN+ReLU folded (resnet_v2.py:127-128)
            ConvSpec c{un + "/conv1", sc + "/conv1", sc + "/conv1/BatchNorm", sc + "/preact", x, S_T1, g.side_in, g.c_in, g.side_in, g.width};
            c.relu = true;
            p->layers.push_back(conv(c));
        }
        // conv2: conv2d_same 3x3 (resnet_utils.py:82-135).  A sum that stays on chip: conv2's output is read again by the next unit's launch
        const int t2 = f.sum == SumTo::OnChip ? S_T2B : S_T2;
        ConvSpec c2{un + "/conv2", sc + "/conv2", sc + "/conv2/BatchNorm", "", S_T1, t2, g.side_in, g.width, g.side_out, g.width};
        c2.k = 3; c2.stride = g.stride; c2.rate = g.rate; c2.pad_beg = g.pad_beg; c2.relu = true;
        Layer L2 = conv(c2);
        if (f.conv1 == Conv1At::FrontOfConv2) fuse_conv1_in_front(L2, g, x);
        p->layers.push_back(L2);
        // conv3 + bias + shortcut (resnet_v2.py:134-138); a sub-sampled sum: metro_forward_upto stopping here writes the whole sum to S_SC
        ConvSpec c3{un + "/conv3", sc + "/conv3", "", "", t2, f.sum == SumTo::SubSampled ? S_SC : out, g.side_out, g.width, g.side_out, g.c_out};
        if (f.shortcut == ShortcutFrom::OwnLaunch || f.shortcut == ShortcutFrom::Pair) {
            c3.res_slot = S_SC; c3.res_side = g.side_out;
        } else if (f.shortcut == ShortcutFrom::Identity || f.shortcut == ShortcutFrom::Compact) {
            c3.res_slot = x; c3.res_side = g.side_in; c3.res_stride = g.stride; c3.res_offset = g.shift;
        }
        Layer L3 = conv(c3);
        if (f.shortcut == ShortcutFrom::Compact) {
            // the launch adds the compact copy pixel for pixel (the info keeps the reference's gather: stride s, offset shift)
            L3.cd.res_h = L3.cd.res_w = g.side_out; L3.cd.res_stride = 1; L3.cd.res_offset = 0;
            L3.info.fused_flags |= METRO_FUSED_COMPACT_SHORTCUT;
        } else if (f.shortcut == ShortcutFrom::InConv3) {
            fuse_projection_shortcut(L3, g, x);
        } else if (f.shortcut == ShortcutFrom::RebuiltInConv3) {
            // identity shortcut x_1 (resnet_v2.py:120-121 with stride 1) rebuilt in the launch from the previous unit's conv3 launch
            const Layer& L1 = p->layers[prev3];
            L3.info.has_residual = 1;                          // the reference's shortcut, as for any unit
            L3.info.fused_flags |= METRO_FUSED_REBUILT_SHORTCUT; L3.form = LayerForm::NextRebuild;
            L3.reb.w = L1.main.w; L3.reb.bias = L1.main.bias; L3.reb_slot = L1.in_slot;
            L3.psc = L1.psc; L3.psc_slot = L1.psc_slot;
        }
        if (f.sum != SumTo::Stored) L3.info.fused_flags |= METRO_FUSED_OUT_ON_CHIP;
        L3.out_mode = f.sum == SumTo::Stored ? 0 : f.sum == SumTo::OnChip ? 1 : 2;
        if (f.sum == SumTo::SubSampled) { L3.sub_slot = out; L3.sub_off = f.sub_off; L3.sub_side = f.sub_side; }
        if (f.carries_next_conv1) fuse_next_conv1(L3, *next_unit);
        p->layers.push_back(L3);
        prev3 = (int)p->layers.size() - 1;
        *x_slot = out;
        return METRO_OK;
    }
};

void layout_workspace(MetroPlan* p, bool head_fused);

int build_plan(MetroPlan* p) {
    const MetroSpec& sp = p->spec;
    Builder B{p, std::string("MainPart/resnet_v2_") + std::to_string(sp.arch)};
    const bool fast = p->fast;
    const int adt = p->act_dtype, aes = p->act_bytes, side = sp.proc_side, bw = sp.base_width;

    // ---- root block: conv1 7x7/2 with explicit pad 3 (+bias, no BN, no ReLU), pool1 ----------
    // reference resnet_v2.py:219-224, resnet_utils.py:125-135,177-185
    const int s2 = stem_side(side), s4 = pool_side(s2);
    bool fused_stem_pool = false;
    // the fused stem+pool kernel can read the fp32 crops directly (cast + border on the way into LDS)
    const bool raw_stem = fast && stem_pool_f32in_supported(side, bw);
    if (fast && !raw_stem) {
        Layer L;
        L.kind = LK_PREP;
        L.cd.h_in = L.cd.w_in = side; L.cd.c_in = 3;
        L.cd.h_out = side + 6; L.cd.w_out = side + 8; L.cd.c_out = 4; L.cd.out_dtype = METRO_F16;
        L.in_slot = S_IMAGES; L.out_slot = S_PREP;
        B.need(S_PREP, (int64_t)(side + 6) * (side + 8) * 4 * 2);
        B.fill_info(L, "prep_input", 0.0);
        p->layers.push_back(L);
    }
    if (fast) {
        // stem as a pad-free 7x1-tap conv over the bordered 4-channel image: each tap = 8 pixels x 4 channels = 32 contiguous
        // fp16; weights packed [c_out][7][8][4] (zeros in the 8th pixel and the 4th channel).
        Layer S;
        MetroConvDesc& cd = S.cd;
        cd.h_in = side + 6; cd.w_in = side + 8; cd.c_in = 32; cd.in_pix_stride = 4;
        cd.h_out = cd.w_out = s2; cd.c_out = bw;
        cd.kh = 7; cd.kw = 1; cd.stride = 2; cd.dilation = 1; cd.pad_top = cd.pad_left = 0;
        cd.out_dtype = adt; cd.in_dtype = METRO_F16;
        const std::string cv = B.root + "/conv1";
        S.main.w = B.add_param("conv1/W", METRO_PARAM_CONV_W, cv, "", METRO_F16, {bw, 7, 7, 3, 8, 4});
        S.main.bias = B.add_param("conv1/bias", METRO_PARAM_BIAS, cv, "", METRO_F32, {bw});
        S.in_slot = S_PREP; S.out_slot = S_STEM;
        if (stem_pool_f16_supported(side, bw)) {
            // reference resnet_v2.py:219-224: the pooled tensor is the only thing block1 reads
            fused_stem_pool = true;
            S.form = raw_stem ? LayerForm::StemPoolF32In : LayerForm::StemPool;
            if (raw_stem) S.in_slot = S_IMAGES;
            S.out_slot = S_X0;
            B.need(S_X0, (int64_t)s4 * s4 * bw * aes);
            B.fill_info(S, "conv1+pool1", 2.0 * s2 * s2 * bw * 7 * 7 * 3);
            S.info.h_out = S.info.w_out = s4;
            S.cd.h_out = S.cd.w_out = s4;         // shape of the stored tensor (forward_upto, out_bytes_per_image)
        } else {
            B.need(S_STEM, (int64_t)s2 * s2 * bw * aes);
            B.fill_info(S, "conv1", 2.0 * s2 * s2 * bw * 7 * 7 * 3);
        }
        p->layers.push_back(S);
    } else {
        ConvSpec c{"conv1", "conv1", "", "", S_IMAGES, S_STEM, side, 3, s2, bw};
        c.k = 7; c.stride = 2; c.pad_beg = 3; c.in_dtype = METRO_F32;
        p->layers.push_back(B.conv(c));
    }
    if (!fused_stem_pool) {
        Layer L;
        L.kind = LK_POOL;
        L.cd.h_in = L.cd.w_in = s2; L.cd.c_in = bw; L.cd.h_out = L.cd.w_out = s4; L.cd.c_out = bw;
        L.cd.kh = L.cd.kw = 3; L.cd.stride = 2; L.cd.dilation = 1; L.cd.pad_top = L.cd.pad_left = 1;
        L.cd.out_dtype = adt;
        L.in_slot = S_STEM; L.out_slot = S_X0;
        B.need(S_X0, (int64_t)s4 * s4 * bw * aes);
        B.fill_info(L, "pool1", 0.0);
        p->layers.push_back(L);
    }

    // ---- the bottleneck units -----------------------------------------------------------------
    std::vector<UnitGeom> units;
    std::vector<UnitFusion> fusions;
    int st = unit_geometry(sp, &units);
    if (st == METRO_OK) st = choose_fusion(units, fast, &fusions);
    int cur = S_X0;
    for (size_t i = 0; i < units.size() && st == METRO_OK; ++i)
        st = B.emit_unit(units[i], fusions[i], i + 1 < units.size() ? &units[i + 1] : nullptr, &cur);
    if (st != METRO_OK) return st;
    const int cur_side = units.back().side_out, cur_c = units.back().c_out;

    // ---- postnorm (prologue) + logits 1x1 (+bias), fp32 out (resnet_v2.py:229-236, architectures.py:34)
    const int c_head = sp.depth * sp.n_joints_head;
    ConvSpec lg{"logits", "logits", "", "postnorm", cur, S_LOGITS, cur_side, cur_c, cur_side, c_head};
    lg.out_dtype = sp.precision == METRO_PREC_F64 ? METRO_F64 : METRO_F32;
    Layer logits = B.conv(lg);
    // fp16 mode: the logits stay on chip (volumetric.py:227-235 starts in the GEMM's epilogue)
    const bool head_fused = fast && head_f16_supported(cur_c, c_head, sp.n_joints_head, sp.depth, cur_side);
    if (head_fused) logits.form = LayerForm::Head;
    p->head_fused = head_fused;
    p->layers.push_back(logits);

    // ---- soft-argmax + decode ---------------------------------------------------------------
    Layer L;
    L.kind = LK_SOFTARGMAX;
    L.cd.h_in = L.cd.w_in = cur_side; L.cd.c_in = c_head; L.cd.h_out = 1; L.cd.w_out = sp.n_joints_out;
    L.cd.c_out = 3; L.cd.out_dtype = METRO_F32;
    L.in_slot = S_LOGITS;
    L.form = head_fused ? LayerForm::Head : LayerForm::Plain;
    L.head_c_in = cur_c;
    B.fill_info(L, "softargmax", 0.0);
    p->layers.push_back(L);

    layout_workspace(p, head_fused);
    return METRO_OK;
}

// slot offsets, and what each layer's info says about where its outputs are and what the launch touches
void layout_workspace(MetroPlan* p, bool head_fused) {
    const MetroSpec& sp = p->spec;
    const bool fast = p->fast;
    int64_t off = 0, aes = p->act_bytes;
    for (int s = 0; s < S_COUNT; ++s) {
        p->slot_offset[s] = off;
        int64_t bytes = p->slot_bytes_per_image[s] * p->max_batch;
        if (s == S_PART) {
            const int hs = sp.proc_side / sp.stride;
            bytes = softargmax_scratch_bytes(p->max_batch, hs, sp.n_joints_head);
            // the one-launch head writes one (m, S, Sx, Sy, Sz) fp32 record per (image, 64-pixel slab, joint): more slabs
            // than the two-launch path's <= 64 once the heat map has > 4096 pixels (side >= 96, e.g. proc_side 384 at stride 4)
            if (head_fused)
                bytes = std::max(bytes, (int64_t)p->max_batch * head_f16_slabs(hs) * sp.n_joints_head * 5 * 4);
        }
        if (s == S_STATUS) bytes = (int64_t)p->max_batch * 4;      // int32 per image: the finalize launch's non-finite screen
        off = align_up(off + bytes, 256);
    }
    p->workspace_bytes = off;
    for (Layer& L : p->layers) {
        L.info.out_offset = L.out_slot >= 0 ? p->slot_offset[L.out_slot] : -1;
        L.info.out_sub_offset = L.out_mode == 2 ? p->slot_offset[L.sub_slot] : -1;
        L.info.out_sub_side = L.out_mode == 2 ? L.sub_side : 0;
        L.info.out_sub_off = L.out_mode == 2 ? L.sub_off : 0;
        const int64_t es = dtype_bytes(L.cd.out_dtype);
        L.info.out_bytes_per_image = (int64_t)L.cd.h_out * L.cd.w_out * (L.form == LayerForm::Pair ? L.cd.c_out - L.c2 : L.cd.c_out) * es;
        const bool two = L.out2_slot != S_NONE;
        L.info.out2_offset = two ? p->slot_offset[L.out2_slot] : -1;
        L.info.out2_channels = two ? L.c2 : 0;
        if (L.form == LayerForm::Conv1Conv2) {  // conv1's output is a DUMP-ONLY second tensor (metro_forward_upto stopping here), not traffic
            L.info.out2_offset = p->slot_offset[S_T1];
            L.info.out2_channels = p->params[L.conv1.w].c_out;
        }
        // algorithmic bytes: every tensor the launch touches, once
        const int64_t in_es = L.in_slot == S_IMAGES ? 4 : (L.kind == LK_SOFTARGMAX ? (sp.precision == METRO_PREC_F64 ? 8 : 4)
                                                           : (L.kind == LK_CONV && !fast ? aes : (L.kind == LK_CONV ? 2 : aes)));
        int64_t act = 0;
        if (L.in_slot == S_IMAGES) act += (int64_t)sp.proc_side * sp.proc_side * 3 * 4;
        else if (L.kind == LK_CONV && L.cd.in_pix_stride != L.cd.c_in) act += (int64_t)L.cd.h_in * L.cd.w_in * L.cd.in_pix_stride * in_es;
        else act += (int64_t)L.cd.h_in * L.cd.w_in * L.cd.c_in * in_es;
        if (L.kind == LK_SOFTARGMAX) act += (int64_t)sp.n_joints_out * 3 * 4;
        else if (L.out_mode == 0) act += L.info.out_bytes_per_image;
        else if (L.out_mode == 2) act += (int64_t)L.sub_side * L.sub_side * L.cd.c_out * es;     // the sub-sampled copy only
        if (L.reb.w >= 0) act += (int64_t)L.cd.h_out * L.cd.w_out * p->params[L.reb.w].c_in * es;  // the previous unit's conv2 output
        if (two) act += (int64_t)L.cd.h_out * L.cd.w_out * L.info.out2_channels * es;
        if (L.kind == LK_CONV && L.cd.has_residual) act += (int64_t)L.cd.h_out * L.cd.w_out * L.cd.c_out * es;
        if (L.psc.w >= 0) act += (int64_t)L.cd.h_out * L.cd.w_out * p->params[L.psc.w].c_in * es;      // the unit input, read for the shortcut
        if (L.form == LayerForm::Head) {       // logits never reach HBM: the launch writes / the finalize reads the per-slab statistics
            const int64_t part = (int64_t)head_f16_slabs(sp.proc_side / sp.stride) * sp.n_joints_head * 5 * 4;
            if (L.kind == LK_CONV) act = (int64_t)L.cd.h_in * L.cd.w_in * L.cd.c_in * 2 + part;
            else act = part + (int64_t)sp.n_joints_out * 3 * 4;
        }
        L.info.algo_act_bytes_per_image = act;
        int64_t pb = 0;
        for (const ConvParams& g : {L.main, L.conv1, L.next, L.psc, L.reb})
            for (int idx : {g.w, g.bias, g.scale, g.shift})
                if (idx >= 0) pb += p->params[idx].bytes;
        L.info.algo_param_bytes = pb;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
extern "C" {

int metro_plan_create(const MetroSpec* spec, int32_t max_batch, MetroPlan** out_plan) {
    METRO_CHECK_ARG(spec != nullptr && out_plan != nullptr, "metro_plan_create: NULL argument");
    *out_plan = nullptr;
    METRO_CHECK_ARG(spec->arch == 50 || spec->arch == 101, "unsupported arch %d (50|101)", spec->arch);
    METRO_CHECK_ARG(spec->stride == 4 || spec->stride == 8 || spec->stride == 16 || spec->stride == 32,
                    "unsupported stride %d (4|8|16|32)", spec->stride);
    METRO_CHECK_ARG(spec->proc_side > 0 && spec->proc_side % 32 == 0, "proc_side %d must be a positive multiple of 32", spec->proc_side);
    // the soft-argmax places pixel i at i / (side - 1): a 1 x 1 heat map has no coordinate
    METRO_CHECK_ARG(spec->proc_side / spec->stride >= 2, "heat-map side %d (proc_side %d / stride %d) must be >= 2",
                    spec->proc_side / spec->stride, spec->proc_side, spec->stride);
    METRO_CHECK_ARG(spec->depth >= 2 && spec->depth <= 64, "depth %d out of range", spec->depth);
    METRO_CHECK_ARG(spec->n_joints_head >= 1 && spec->n_joints_head <= METRO_MAX_JOINTS, "n_joints_head %d out of range", spec->n_joints_head);
    METRO_CHECK_ARG(spec->n_joints_out >= 1 && spec->n_joints_out <= METRO_MAX_JOINTS, "n_joints_out %d out of range", spec->n_joints_out);
    for (int i = 0; i < spec->n_joints_out; ++i)
        METRO_CHECK_ARG(spec->permutation[i] >= 0 && spec->permutation[i] < spec->n_joints_head,
                        "permutation[%d] = %d outside the head's %d joints", i, spec->permutation[i], spec->n_joints_head);
    METRO_CHECK_ARG((spec->depth * spec->n_joints_head) % 4 == 0, "depth*n_joints_head must be a multiple of 4");
    METRO_CHECK_ARG(spec->precision == METRO_PREC_F16 || spec->precision == METRO_PREC_F32 || spec->precision == METRO_PREC_F64 ||
                        spec->precision == METRO_PREC_F32M, "unknown precision %d", spec->precision);
    METRO_CHECK_ARG(spec->base_width >= 8 && spec->base_width % 8 == 0, "base_width %d must be a positive multiple of 8", spec->base_width);
    METRO_CHECK_ARG(max_batch >= 1 && max_batch <= 4096, "max_batch %d out of range", max_batch);
    METRO_CHECK_ARG(spec->box_size_mm > 0.f, "box_size_mm must be positive");

    MetroPlan* p = new MetroPlan();
    p->spec = *spec;
    p->max_batch = max_batch;
    p->fast = spec->precision == METRO_PREC_F16;
    const bool f32_store = spec->precision == METRO_PREC_F32 || spec->precision == METRO_PREC_F32M;
    p->act_dtype = p->fast ? METRO_F16 : f32_store ? METRO_F32 : METRO_F64;
    p->act_bytes = p->fast ? 2 : f32_store ? 4 : 8;
    const int st = build_plan(p);
    if (st != METRO_OK) { delete p; return st; }
    *out_plan = p;
    return METRO_OK;
}

int metro_plan_destroy(MetroPlan* plan) {
    if (plan)
        for (GraphEntry& g : plan->graphs)
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (plan && plan->cap_stream) (void)hipStreamDestroy(plan->cap_stream);
    delete plan;
    return METRO_OK;
}
int64_t metro_plan_workspace_bytes(const MetroPlan* plan) { return plan ? plan->workspace_bytes : -1; }
int64_t metro_plan_param_bytes(const MetroPlan* plan) { return plan ? plan->param_bytes : -1; }
int32_t metro_plan_num_params(const MetroPlan* plan) { return plan ? (int32_t)plan->params.size() : -1; }
int32_t metro_plan_num_layers(const MetroPlan* plan) { return plan ? (int32_t)plan->layers.size() : -1; }
double metro_plan_flops_per_image(const MetroPlan* plan) { return plan ? plan->flops_per_image : -1.0; }

int metro_plan_param_info(const MetroPlan* plan, int32_t index, MetroParamInfo* out) {
    METRO_CHECK_ARG(plan && out && index >= 0 && index < (int)plan->params.size(), "metro_plan_param_info: bad argument");
    *out = plan->params[index];
    return METRO_OK;
}

int metro_plan_layer_info(const MetroPlan* plan, int32_t index, MetroLayerInfo* out) {
    METRO_CHECK_ARG(plan && out && index >= 0 && index < (int)plan->layers.size(), "metro_plan_layer_info: bad argument");
    *out = plan->layers[index].info;
    return METRO_OK;
}

int64_t metro_plan_status_offset(const MetroPlan* plan) { return plan ? plan->slot_offset[S_STATUS] : -1; }

}  // extern "C"
