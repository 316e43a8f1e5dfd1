// Next-frame person boxes from the track table, on the device (metro_predict_boxes, include/metro_hip.h, which is the
// specification).  Nothing in the reference to restate: one example is one image and its box is given.  Between key frames of a
// detector the next crop is cut around where the tracked person is about to be: every live slot of the table
// metro_associate_tracks walks is advanced to the exposure's time by smooth_predict (smooth_step.h, the function the association
// compares boxes against), its joints go through the frame's calibrated, lens-distorted camera, and the union of the joints'
// pixel intervals is the box.  Two launches on one stream:
//   predict_boxes_kernel   one thread per (frame, slot), 64 per block: the dense tables boxes [F][T][4] (NaN: no box) and
//                          joints [F][T] (visible joints, -1: free or too old)
//   compact_boxes_kernel   one workgroup of 256: the boxes present, frame-major then by slot, then the detector's boxes that
//                          no predicted box of their frame covers, into rows in that order -- chunks of 256 with a running
//                          base, the position of a row from a wave ballot and popcount plus the per-wave sums in LDS
// Every step is a __host__ __device__ function of one index, so tests/test_predict_boxes.py runs the same code on the host with
// one thread and a running count where the kernel has the ballots.  One thread per (frame, slot), every matrix in scalar
// registers and every loop over P with constant bounds: nothing is indexed dynamically but global memory (no scratch).
// World -> camera is Camera.world_to_camera, R (p - t), from the fp32 table entries in fp64; the pixel is project_points' fp32
// chain in its statement order; the margin and the box are fp64.  No FMA contraction.
#include "metro_common.h"
#include "smooth_step.h"

#pragma clang fp contract(off)

namespace metro {

constexpr int PREDICT_THREADS = 64;
constexpr int COMPACT_THREADS = 256;
constexpr int PREDICT_MAX_DETECTIONS = METRO_PREDICT_MAX_DETECTIONS;

struct PredictArgs {
    const double* state;              // [T][J][28], read only
    const int* ids;                   // [T], read only
    const MetroFrameCamera* cameras;  // [n_cameras]: 1 (every frame) or F
    const double* det_boxes;          // [m][4] or null
    const int* det_frame;             // [m] or null
    double* boxes_dense;              // [F][T][4]
    int* joints_dense;                // [F][T]
    double* boxes_out;                // [F T + m][4]
    int* frame_out;                   // [F T + m]
    int* slot_out;
    int* id_out;
    int* detection_out;
    int* n_joints_out;
    int* counts;                      // [5]: rows, predicted, suppressed, bad detections, bad frame indices
    int n_tracks, n_out, n_cameras, n_frames, n_det, coords, min_joints, clip;
    double q, max_age, expand, n_sigma, max_sigma, near, min_side, iou_max;
    double t_frame[METRO_MAX_FRAMES];       // [F] s, the host's values in the kernel arguments
    int sizes[METRO_MAX_FRAMES * 2];        // [F][2] (W, H), likewise
};

// verdicts of a detection
constexpr int DET_KEPT = 0, DET_SUPPRESSED = 1, DET_BAD = 2, DET_BAD_FRAME = 3;

// project_points (cameralib.py:375-397) in its statement order, fp32; without coefficients K (x/z, y/z, 1).  The chain is
// distort_normalized's (camera_math.h), written out: through the call hipcc emits another instruction stream for
// predict_boxes_kernel (same values, other schedule and registers), and a site is folded only where the kernel stays identical.
__host__ __device__ inline void predict_project(const MetroFrameCamera& c, float x, float y, float z, float& u, float& v) {
    float px = x / z, py = y / z;
    if (c.has_distortion) {
        const float* d = c.distortion;              // k1 k2 p1 p2 k3
        const float r2 = px * px + py * py;
        const float r4 = r2 * r2;
        float dist = d[0] * r2;
        dist += d[1] * r4;
        const float r6 = r4 * r2;
        dist += d[4] * r6;
        dist += 1.f;
        dist += px * (2.f * d[3]);
        dist += py * (2.f * d[2]);
        px = px * dist;
        px = px + r2 * d[3];
        py = py * dist;
        py = py + r2 * d[2];
    }
    const float* K = c.intrinsics;
    u = (K[0] * px + K[1] * py) + K[2];
    v = (K[3] * px + K[4] * py) + K[5];
}

// the pixel interval of one predicted joint m on camera c; false: not visible
__host__ __device__ inline bool predict_joint(const PredictArgs& a, const MetroFrameCamera& c, const SmoothKf& m, double& u0,
                                              double& u1, double& v0, double& v1) {
    double x = m.x[0], y = m.x[1], z = m.x[2];
    if (a.coords == METRO_COORDS_WORLD) {            // Camera.world_to_camera: (p - t) @ R.T
        const double d0 = x - (double)c.t[0], d1 = y - (double)c.t[1], d2 = z - (double)c.t[2];
        x = ((double)c.r[0] * d0 + (double)c.r[1] * d1) + (double)c.r[2] * d2;
        y = ((double)c.r[3] * d0 + (double)c.r[4] * d1) + (double)c.r[5] * d2;
        z = ((double)c.r[6] * d0 + (double)c.r[7] * d1) + (double)c.r[8] * d2;
    }
    if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z)) || !(z >= a.near)) return false;
    if (c.has_distortion) {                          // the radial polynomial still grows here: d/dr of r (1 + k1 r^2 + ...)
        const double nx = x / z, ny = y / z;
        const double r2 = nx * nx + ny * ny;
        const double k1 = c.distortion[0], k2 = c.distortion[1], k3 = c.distortion[4];
        const double slope = ((1.0 + (3.0 * k1) * r2) + (5.0 * k2) * (r2 * r2)) + (7.0 * k3) * ((r2 * r2) * r2);
        if (!(slope > 0.0)) return false;
    }
    float u, v;
    predict_project(c, (float)x, (float)y, (float)z, u, v);
    if (!(__builtin_isfinite(u) && __builtin_isfinite(v))) return false;
    double var = SMOOTH_P(m.p, 0, 0);
    if (SMOOTH_P(m.p, 1, 1) > var) var = SMOOTH_P(m.p, 1, 1);
    if (SMOOTH_P(m.p, 2, 2) > var) var = SMOOTH_P(m.p, 2, 2);
    double sigma = sqrt(var > 0.0 ? var : 0.0);
    if (!(sigma <= a.max_sigma)) sigma = a.max_sigma;
    const double mg = ((a.n_sigma * sigma) * sqrt(fabs((double)c.intrinsics[0] * (double)c.intrinsics[4]))) / z;
    u0 = (double)u - mg; u1 = (double)u + mg;
    v0 = (double)v - mg; v1 = (double)v + mg;
    return true;
}

// item idx = f T + s of the dense tables
__host__ __device__ inline void predict_one(const PredictArgs& a, int idx) {
    const int f = idx / a.n_tracks, s = idx - f * a.n_tracks;
    const double nan = __builtin_nan("");
    double* box = a.boxes_dense + (size_t)idx * 4;
    box[0] = box[1] = box[2] = box[3] = nan;
    a.joints_dense[idx] = -1;
    if (a.ids[s] < 0) return;
    const double* st = a.state + (size_t)s * a.n_out * SMOOTH_STATE_DOUBLES;
    const double t = a.t_frame[f];
    bool live = false;
    double seen = -__builtin_inf();
    for (int j = 0; j < a.n_out; ++j) {
        const double tl = st[(size_t)j * SMOOTH_STATE_DOUBLES + 27];
        if (tl != tl) continue;
        live = true;
        if (tl > seen) seen = tl;
    }
    if (!live || t - seen > a.max_age) return;
    const MetroFrameCamera& c = a.cameras[a.n_cameras == 1 ? 0 : f];
    double x0 = __builtin_inf(), y0 = __builtin_inf(), x1 = -__builtin_inf(), y1 = -__builtin_inf();
    int cnt = 0;
    for (int j = 0; j < a.n_out; ++j) {
        SmoothKf k, m;
        double tl = 0.0;
        if (!smooth_state_load(st + (size_t)j * SMOOTH_STATE_DOUBLES, k, tl)) continue;
        double dt = t - tl;
        if (!(dt > 0.0)) dt = 0.0;                   // as the association takes it
        smooth_predict(k, dt, a.q, m);
        double u0, u1, v0, v1;
        if (!predict_joint(a, c, m, u0, u1, v0, v1)) continue;
        if (u0 < x0) x0 = u0;
        if (u1 > x1) x1 = u1;
        if (v0 < y0) y0 = v0;
        if (v1 > y1) y1 = v1;
        ++cnt;
    }
    a.joints_dense[idx] = cnt;
    if (cnt < a.min_joints) return;
    const double cx = (x0 + x1) / 2, cy = (y0 + y1) / 2;
    const double hw = ((x1 - x0) / 2) * a.expand, hh = ((y1 - y0) / 2) * a.expand;
    x0 = cx - hw; x1 = cx + hw;
    y0 = cy - hh; y1 = cy + hh;
    if (a.clip) {
        const double w = a.sizes[f * 2], h = a.sizes[f * 2 + 1];
        if (x0 < 0.0) x0 = 0.0;
        if (y0 < 0.0) y0 = 0.0;
        if (x1 > w) x1 = w;
        if (y1 > h) y1 = h;
    }
    const double bw = x1 - x0, bh = y1 - y0;
    if (!(bw >= a.min_side && bh >= a.min_side)) return;
    box[0] = x0; box[1] = y0; box[2] = bw; box[3] = bh;
}

__host__ __device__ inline bool compact_present(const PredictArgs& a, int idx) {
    const double x = a.boxes_dense[(size_t)idx * 4];
    return x == x;
}

__host__ __device__ inline void compact_write_predicted(const PredictArgs& a, int idx, int at) {
    const int f = idx / a.n_tracks, s = idx - f * a.n_tracks;
    for (int e = 0; e < 4; ++e) a.boxes_out[(size_t)at * 4 + e] = a.boxes_dense[(size_t)idx * 4 + e];
    a.frame_out[at] = f;
    a.slot_out[at] = s;
    a.id_out[at] = a.ids[s];
    a.detection_out[at] = -1;
    a.n_joints_out[at] = a.joints_dense[idx];
}

// what becomes of detection k: a frame outside [0, F) first, then its own coordinates, then the predicted boxes of its frame
__host__ __device__ inline int compact_detection(const PredictArgs& a, int k) {
    const int f = a.det_frame[k];
    if ((unsigned)f >= (unsigned)a.n_frames) return DET_BAD_FRAME;
    const double* d = a.det_boxes + (size_t)k * 4;
    const double x = d[0], y = d[1], w = d[2], h = d[3];
    if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(w) && __builtin_isfinite(h)) || !(w > 0.0) || !(h > 0.0))
        return DET_BAD;
    for (int s = 0; s < a.n_tracks; ++s) {
        const double* p = a.boxes_dense + ((size_t)f * a.n_tracks + s) * 4;
        if (p[0] != p[0]) continue;
        const double lo_x = p[0] > x ? p[0] : x, hi_x = p[0] + p[2] < x + w ? p[0] + p[2] : x + w;
        const double lo_y = p[1] > y ? p[1] : y, hi_y = p[1] + p[3] < y + h ? p[1] + p[3] : y + h;
        const double ix = hi_x - lo_x, iy = hi_y - lo_y;
        const double inter = ix > 0.0 && iy > 0.0 ? ix * iy : 0.0;
        const double uni = (p[2] * p[3] + w * h) - inter;
        if (inter / uni >= a.iou_max) return DET_SUPPRESSED;
    }
    return DET_KEPT;
}

__host__ __device__ inline void compact_write_detection(const PredictArgs& a, int k, int at) {
    for (int e = 0; e < 4; ++e) a.boxes_out[(size_t)at * 4 + e] = a.det_boxes[(size_t)k * 4 + e];
    a.frame_out[at] = a.det_frame[k];
    a.slot_out[at] = -1;
    a.id_out[at] = -1;
    a.detection_out[at] = k;
    a.n_joints_out[at] = -1;
}

__global__ __launch_bounds__(PREDICT_THREADS) void predict_boxes_kernel(PredictArgs a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < a.n_frames * a.n_tracks) predict_one(a, idx);
}

// where this thread's row goes among the kept rows of the chunk, and the chunk's total: a ballot and popcount within the wave,
// the per-wave sums through LDS.  Called by all 256 threads; the barrier at the end frees wave_sum for the next chunk.
__device__ inline int compact_position(bool keep, int* wave_sum, int tid, int& total) {
    const unsigned long long b = __ballot(keep);
    const int lane = tid & 63, wave = tid >> 6;
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_sum[wave] = __popcll(b);
    __syncthreads();
    int at = before;
    total = 0;
    for (int w = 0; w < COMPACT_THREADS / 64; ++w) {
        if (w < wave) at += wave_sum[w];
        total += wave_sum[w];
    }
    __syncthreads();
    return at;
}

__global__ __launch_bounds__(COMPACT_THREADS) void compact_boxes_kernel(PredictArgs a) {
    __shared__ int wave_sum[COMPACT_THREADS / 64];
    __shared__ int tally[4];                               // by verdict
    const int tid = threadIdx.x;
    if (tid < 4) tally[tid] = 0;
    __syncthreads();
    const int n_dense = a.n_frames * a.n_tracks;
    int base = 0;
    for (int c0 = 0; c0 < n_dense; c0 += COMPACT_THREADS) {   // every thread takes every trip: the barriers inside
        const int idx = c0 + tid;
        const bool keep = idx < n_dense && compact_present(a, idx);
        int total;
        const int at = base + compact_position(keep, wave_sum, tid, total);
        if (keep) compact_write_predicted(a, idx, at);
        base += total;
    }
    const int n_predicted = base;
    for (int c0 = 0; c0 < a.n_det; c0 += COMPACT_THREADS) {
        const int k = c0 + tid;
        int verdict = -1;
        if (k < a.n_det) {
            verdict = compact_detection(a, k);
            if (verdict != DET_KEPT) atomicAdd(&tally[verdict], 1);
        }
        int total;
        const int at = base + compact_position(verdict == DET_KEPT, wave_sum, tid, total);
        if (verdict == DET_KEPT) compact_write_detection(a, k, at);
        base += total;
    }
    __syncthreads();
    if (tid == 0) {
        a.counts[0] = base;
        a.counts[1] = n_predicted;
        a.counts[2] = tally[DET_SUPPRESSED];
        a.counts[3] = tally[DET_BAD];
        a.counts[4] = tally[DET_BAD_FRAME];
    }
}

// frame_sizes [F][2] and frame_times [F] are HOST arrays, copied into the arguments (F <= METRO_MAX_FRAMES)
PredictArgs make_predict_args(const double* state, const int* ids, int n_tracks, int n_out, const MetroFrameCamera* cameras,
                              int n_cameras, const int* frame_sizes, const double* frame_times, int n_frames, int coords, double q,
                              double max_age, double expand, double n_sigma, double max_sigma, double near, double min_side,
                              int min_joints, int clip, const double* det_boxes, const int* det_frame, int n_det, double iou_max,
                              double* boxes_dense, int* joints_dense, double* boxes_out, int* frame_out, int* slot_out, int* id_out,
                              int* detection_out, int* n_joints_out, int* counts) {
    PredictArgs a;
    a.state = state; a.ids = ids; a.cameras = cameras; a.det_boxes = det_boxes; a.det_frame = det_frame;
    a.boxes_dense = boxes_dense; a.joints_dense = joints_dense; a.boxes_out = boxes_out; a.frame_out = frame_out;
    a.slot_out = slot_out; a.id_out = id_out; a.detection_out = detection_out; a.n_joints_out = n_joints_out; a.counts = counts;
    a.n_tracks = n_tracks; a.n_out = n_out; a.n_cameras = n_cameras; a.n_frames = n_frames; a.n_det = n_det;
    a.coords = coords; a.min_joints = min_joints; a.clip = clip != 0;
    a.q = q; a.max_age = max_age; a.expand = expand; a.n_sigma = n_sigma; a.max_sigma = max_sigma; a.near = near;
    a.min_side = min_side; a.iou_max = iou_max;
    for (int f = 0; f < METRO_MAX_FRAMES; ++f) {
        const bool in = f < n_frames;
        a.t_frame[f] = in ? frame_times[f] : 0.0;
        a.sizes[f * 2] = in ? frame_sizes[f * 2] : 1;
        a.sizes[f * 2 + 1] = in ? frame_sizes[f * 2 + 1] : 1;
    }
    return a;
}

int launch_predict_boxes(const PredictArgs& a, hipStream_t stream) {
    if (note_kernel("predict_boxes")) return METRO_OK;
    const int n_dense = a.n_frames * a.n_tracks;
    hipLaunchKernelGGL(predict_boxes_kernel, dim3((n_dense + PREDICT_THREADS - 1) / PREDICT_THREADS), dim3(PREDICT_THREADS), 0, stream, a);
    hipLaunchKernelGGL(compact_boxes_kernel, dim3(1), dim3(COMPACT_THREADS), 0, stream, a);
    return launch_status("predict_boxes");
}

}  // namespace metro

extern "C" int metro_predict_boxes(const double* d_state, const int32_t* d_ids, int32_t n_tracks, int32_t n_joints_out,
                                   const MetroFrameCamera* d_cameras, int32_t n_cameras, const int32_t* frame_sizes,
                                   const double* frame_times, int32_t n_frames, int32_t coords, double q, double max_age_s,
                                   double expand, double n_sigma, double max_sigma_mm, double near_mm, double min_side_px,
                                   int32_t min_joints, int32_t clip, const double* d_det_boxes, const int32_t* d_det_frame,
                                   int32_t n_detections, double iou_max, double* d_boxes_dense, int32_t* d_joints_dense,
                                   double* d_boxes_out, int32_t* d_frame_out, int32_t* d_slot_out, int32_t* d_id_out,
                                   int32_t* d_detection_out, int32_t* d_n_joints_out, int32_t* d_counts, void* stream) {
    using namespace metro;
    const auto fin = [](double v) { return __builtin_isfinite(v); };
    METRO_CHECK_ARG(n_joints_out >= 1 && n_joints_out <= METRO_MAX_JOINTS, "predict_boxes: n_joints_out %d out of range [1, %d]",
                    n_joints_out, METRO_MAX_JOINTS);
    METRO_CHECK_ARG(coords == METRO_COORDS_CAMERA || coords == METRO_COORDS_WORLD,
                    "predict_boxes: coords must be METRO_COORDS_CAMERA or METRO_COORDS_WORLD (got %d)", coords);
    METRO_CHECK_ARG(n_tracks >= 0 && n_tracks <= METRO_ASSOC_MAX, "predict_boxes: %d track slots (1 to %d)", n_tracks, METRO_ASSOC_MAX);
    METRO_CHECK_ARG(n_frames >= 0 && n_frames <= METRO_MAX_FRAMES, "predict_boxes: %d frames (1 to %d per launch)", n_frames,
                    METRO_MAX_FRAMES);
    METRO_CHECK_ARG(n_detections >= 0 && n_detections <= PREDICT_MAX_DETECTIONS, "predict_boxes: %d detections (0 to %d)",
                    n_detections, PREDICT_MAX_DETECTIONS);
    METRO_CHECK_ARG(fin(q) && q > 0.0, "predict_boxes: q must be finite and > 0 (got %g)", q);
    METRO_CHECK_ARG(fin(max_age_s) && max_age_s >= 0.0, "predict_boxes: max_age_s must be finite and >= 0 (got %g)", max_age_s);
    METRO_CHECK_ARG(fin(expand) && expand >= 1.0, "predict_boxes: expand must be finite and >= 1 (got %g)", expand);
    METRO_CHECK_ARG(fin(n_sigma) && n_sigma >= 0.0, "predict_boxes: n_sigma must be finite and >= 0 (got %g)", n_sigma);
    METRO_CHECK_ARG(fin(max_sigma_mm) && max_sigma_mm >= 0.0, "predict_boxes: max_sigma_mm must be finite and >= 0 (got %g)",
                    max_sigma_mm);
    METRO_CHECK_ARG(fin(near_mm) && near_mm > 0.0, "predict_boxes: near_mm must be finite and > 0 (got %g)", near_mm);
    METRO_CHECK_ARG(fin(min_side_px) && min_side_px >= 0.0, "predict_boxes: min_side_px must be finite and >= 0 (got %g)", min_side_px);
    METRO_CHECK_ARG(fin(iou_max) && iou_max > 0.0 && iou_max <= 1.0, "predict_boxes: iou_max must lie in (0, 1] (got %g)", iou_max);
    METRO_CHECK_ARG(min_joints >= 1 && min_joints <= n_joints_out, "predict_boxes: min_joints %d outside [1, %d]", min_joints,
                    n_joints_out);
    if ((n_tracks == 0 || n_frames == 0) && n_detections == 0) return METRO_OK;      // no row can come out: nothing to do
    METRO_CHECK_ARG(n_tracks >= 1, "predict_boxes: %d track slots (1 to %d)", n_tracks, METRO_ASSOC_MAX);
    METRO_CHECK_ARG(n_frames >= 1, "predict_boxes: %d frames (1 to %d per launch)", n_frames, METRO_MAX_FRAMES);
    METRO_CHECK_ARG(n_cameras == 1 || n_cameras == n_frames,
                    "predict_boxes: %d cameras for %d frames (one for every frame, or one per frame)", n_cameras, n_frames);
    METRO_CHECK_ARG(d_state && d_ids && d_cameras && frame_sizes && frame_times && d_boxes_dense && d_joints_dense && d_boxes_out &&
                        d_frame_out && d_slot_out && d_id_out && d_detection_out && d_n_joints_out && d_counts,
                    "predict_boxes: NULL state / ids / cameras / frame sizes / frame times / output pointer");
    METRO_CHECK_ARG(n_detections == 0 || (d_det_boxes && d_det_frame), "predict_boxes: %d detections with a NULL boxes / frame pointer",
                    n_detections);
    for (int f = 0; f < n_frames; ++f) {
        METRO_CHECK_ARG(frame_sizes[f * 2] >= 1 && frame_sizes[f * 2 + 1] >= 1, "predict_boxes: frame %d is %d x %d pixels", f,
                        frame_sizes[f * 2], frame_sizes[f * 2 + 1]);
        METRO_CHECK_ARG(fin(frame_times[f]), "predict_boxes: the time of frame %d is not finite", f);
    }
    const PredictArgs a = make_predict_args(d_state, d_ids, n_tracks, n_joints_out, d_cameras, n_cameras, frame_sizes, frame_times,
                                            n_frames, coords, q, max_age_s, expand, n_sigma, max_sigma_mm, near_mm, min_side_px,
                                            min_joints, clip, d_det_boxes, d_det_frame, n_detections, iou_max, d_boxes_dense,
                                            d_joints_dense, d_boxes_out, d_frame_out, d_slot_out, d_id_out, d_detection_out,
                                            d_n_joints_out, d_counts);
    return launch_predict_boxes(a, static_cast<hipStream_t>(stream));
}
