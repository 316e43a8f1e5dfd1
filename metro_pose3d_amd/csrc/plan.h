// The plan: what planner.cpp builds and executor.cpp runs.  Private to these two translation units.
#pragma once
#include <cstring>
#include <vector>

#include "metro_common.h"

namespace metro {

enum LayerKind { LK_PREP = 0, LK_CONV = 1, LK_POOL = 2, LK_SOFTARGMAX = 3 };
enum Slot { S_IMAGES = -2, S_NONE = -1, S_PREP = 0, S_STEM, S_X0, S_X1, S_T1, S_T2, S_T2B, S_SC, S_LOGITS, S_PART, S_STATUS, S_COUNT };

inline int dtype_bytes(int dtype) { return dtype == METRO_F16 ? 2 : dtype == METRO_F32 ? 4 : 8; }

struct ConvParams { int w = -1, bias = -1, scale = -1, shift = -1; };   // parameter indices of one convolution's tensors in the blob, -1 = none

// What a conv layer's launch does; launch_layer switches on it.  Plain ... NextRebuild are the fused conv forms (ConvForm).
enum class LayerForm { Plain, Pair, Next, NextProj, NextRebuild, Conv1Conv2, StemPool, StemPoolF32In, Head };
inline ConvForm conv_form(LayerForm f) { return static_cast<ConvForm>(f); }      // of Plain ... NextRebuild
static_assert((int)LayerForm::Plain == (int)ConvForm::Plain && (int)LayerForm::Pair == (int)ConvForm::Pair &&
              (int)LayerForm::Next == (int)ConvForm::Next && (int)LayerForm::NextProj == (int)ConvForm::NextProj &&
              (int)LayerForm::NextRebuild == (int)ConvForm::NextRebuild, "LayerForm starts with ConvForm's values");

struct Layer {
    Layer() { memset(&info, 0, sizeof(info)); }   // with the public struct's padding (metro_plan_layer_info copies it out)
    MetroLayerInfo info;
    int kind = LK_CONV;
    LayerForm form = LayerForm::Plain;  // Head: also the soft-argmax layer behind a fused head, which then only finalizes
    MetroConvDesc cd{};                 // cd.n is filled per call
    int in_slot = S_NONE, out_slot = S_NONE, res_slot = S_NONE;
    ConvParams main;      // the layer's convolution (Pair: the shortcut rows, which conv1's rows follow in the blob)
    ConvParams conv1;     // conv1 of the unit inside the launch: a Pair's second row block, or in front of conv2 (Conv1Conv2, on the unit's input)
    ConvParams next;      // conv1 of the NEXT unit on the launch's output (Next...)
    ConvParams psc;       // the projection shortcut computed in the launch (NextProj, NextRebuild) from the unit input in psc_slot
    ConvParams reb;       // the PREVIOUS unit's conv3 (w, bias; NextRebuild), whose output in reb_slot rebuilds the identity shortcut
    int c2 = 0, out2_slot = S_NONE;   // the second output (Pair, Next...): channels, slot
    int psc_slot = S_NONE, reb_slot = S_NONE;
    // block1 without its 256-channel residual stream in HBM: what metro_forward does with the launch's sum (0 store, 1 keep
    // on chip, 2 sub-sampled compact copy into sub_slot only) and the geometry of that copy
    int out_mode = 0, sub_slot = S_NONE, sub_off = 0, sub_side = 0;
    int head_c_in = 0;    // soft-argmax layer of a fused head: input channels of the logits GEMM (which head kernel ran)
};

// A captured forward: valid for exactly this (batch, buffers, stream) tuple.
struct GraphEntry {
    int n;
    const void* images;
    const void* poses;
    const void* coords01;    // metro_forward_coords01's output (NULL for metro_forward): baked into the finalize launch
    const void* ws;
    hipStream_t stream;
    hipGraphExec_t exec;
    int eager_runs;          // the first call for a key runs eagerly (lazy one-time setup must not be captured)
};

}  // namespace metro

struct MetroPlan {
    std::vector<metro::GraphEntry> graphs;
    hipStream_t cap_stream = nullptr;   // private stream used only to CAPTURE (the legacy null stream cannot capture)
    int graph_max_batch = 0;   // forwards with n <= this replay a captured hipGraph (0 = always eager)
    MetroSpec spec;
    int max_batch;
    bool fast;                           // precision f16
    int act_dtype;                       // MetroDType of activations in the workspace
    int act_bytes;                       // bytes per activation element in the workspace
    std::vector<MetroParamInfo> params;
    std::vector<metro::Layer> layers;
    int64_t slot_bytes_per_image[metro::S_COUNT] = {}, slot_offset[metro::S_COUNT] = {};
    int64_t workspace_bytes = 0, param_bytes = 0;
    const char* d_params = nullptr;
    double flops_per_image = 0.0;
    // metro_plan_bind_heatmaps: host state a forward reads when it enqueues (scratch == nullptr: nothing bound)
    struct { float* xy = nullptr; float* z = nullptr; void* scratch = nullptr; int max_n = 0; } heat;
    // metro_plan_bind_modes: the same (heat_modes.hip)
    struct { int32_t* voxel = nullptr; float* stats = nullptr; void* scratch = nullptr; int max_n = 0, k = 0, radius = 0; } modes;
    // metro_plan_bind_prior: the same (heat_posterior.hip)
    struct { const float* prior = nullptr; float* post = nullptr; void* scratch = nullptr; int max_n = 0; } prior;
    // metro_plan_bind_track_prior: the same (track_priors.hip writes `prior`, heat_posterior.hip reads it); params is a copy
    struct {
        const double* state = nullptr; const int32_t* slot = nullptr; const double* times = nullptr;
        const MetroPlacement* records = nullptr; const int32_t* mirror = nullptr;
        float* prior = nullptr; int32_t* reason = nullptr; float* post = nullptr; void* scratch = nullptr;
        int capacity = 0, max_n = 0;
        MetroTrackPrior params{};
    } track;
    // metro_plan_bind_view_fusion: the same (view_fusion.hip, behind triangulate.hip's launch when `centres` is NULL); bound
    // while `points` is set
    struct {
        const float* xy = nullptr; const MetroPlacement* records = nullptr; const int32_t* rows = nullptr;
        const int32_t* starts = nullptr; const int32_t* mirror = nullptr; const float* centres = nullptr;
        float* points = nullptr; float* cov = nullptr; float* stats = nullptr; int32_t* info = nullptr; float* centres_out = nullptr;
        int n_rows = 0, n_persons = 0, max_n = 0;
        MetroViewFusion params{};
    } fusion;
    // metro_plan_bind_skeleton_modes: the same (skeleton_modes.hip, behind heat_modes.hip's launch); bound while `prob` is set;
    // edges, params and the rooted schedule are copies
    struct {
        const int32_t* voxel = nullptr; const float* stats = nullptr; const double* lengths = nullptr;
        float* prob = nullptr; int32_t* choice = nullptr; float* info = nullptr; float* coords01_sel = nullptr;
        int k = 0, n_edges = 0, max_n = 0;
        int32_t edges[2 * 63] = {};
        signed char parent[METRO_MAX_JOINTS] = {}, parent_edge[METRO_MAX_JOINTS] = {};
        MetroSkeletonModes params{};
    } skel;
    bool head_fused = false;            // the logits stay on chip (LayerForm::Head)
};
