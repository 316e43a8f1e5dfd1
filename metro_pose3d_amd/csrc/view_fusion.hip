// A person's heat-maps from several cameras, fused on a grid of world points (metro_plan_bind_view_fusion, include/metro_hip.h,
// which holds the definition).  Nothing in the reference to restate: its examples have one camera each.  Per (person p, output
// joint r) a cube of G x G x G world points around the joint's centre (its triangulated point, or one the caller gives); every
// crop row of the person's group gives each point the log of the bilinear value of its xy marginal at the point's projection
// through the crop's virtual camera (a floor where the point leaves the map or lies behind the camera); the mean of the rows'
// logs is the energy E, its softmax the weight of the point.  A wrong peak in one camera meets no peak of the others and
// vanishes from the product.  Written: the mean and the central second moments of the points, the largest weight, the
// agreement (the largest E minus what E would be if every camera's highest cell met in one point), the rows used and whether
// the heaviest point lies on the cube's surface.
//   view_fusion_kernel   one workgroup of 256 threads per (person, output joint); thread t owns the points t, t + 256, ...
// fusion_walk below is the whole body, written for a TEAM as posterior_walk of heat_posterior.hip is: the kernel's team is the
// workgroup (64-lane __shfl_xor ladders, one LDS record per wave, folded in wave order by every thread), the host tests' team
// is one thread (tests/test_view_fusion.py compiles this file for the host and walks it).
// LDS: 512 bytes of wave records, 16 row records (the row's K, rotation, centre, map pointer and largest cell: rows are
// handled in chunks of 16), and E as fp64, 32 KB at G = 16.  A thread reads and writes only its own points of E, consecutive
// doubles over consecutive lanes: a 32-lane half covers one 256-byte bank row per ds_read_b64, free of conflicts.  The row
// records are read at one address by all lanes (a broadcast).  The maps stay in L2 (16 KB each at S = 64).
// Passes over E: the maximum with its lowest index; the normaliser and the first moments; the central second moments (never
// E[x^2] - E[x]^2).  Fixed order, no atomics, nothing indexed dynamically but LDS and global memory (no scratch).  fp64 on the
// stored fp32 inputs, each output rounded to fp32 once.  No FMA contraction.
#include "metro_common.h"
#include "camera_math.h"

#pragma clang fp contract(off)

namespace metro {

constexpr int VF_THREADS = 256;
constexpr int VF_CHUNK = 16;                 // rows staged at a time
constexpr int VF_MAX_GRID = 16;
constexpr int VF_LDS_HEAD = 512;             // wave records: 4 waves x 16 values x 4 bytes, or 4 x 6 x 8
constexpr int VF_LDS_ROWS = 3328;            // the row records end here (13 bank rows), E starts

struct VfRow {
    double k[6];            // the first two rows of K = inv(inv_intrinsics)
    double r[9];            // rot_to_world
    double o[3];            // cam_loc
    const float* map;       // [S][S] of the row's (mirror) joint
    float cmax;             // the map's largest cell; +Inf: a cell is not finite
    int used;               // the row index, the record and the mirror joint are usable
};
static_assert(VF_LDS_HEAD + VF_CHUNK * sizeof(VfRow) <= (size_t)VF_LDS_ROWS, "row records");
constexpr int VF_LDS_BYTES = VF_LDS_ROWS + VF_MAX_GRID * VF_MAX_GRID * VF_MAX_GRID * 8;

struct ViewFusionArgs {
    const float* xy;              // [max_n][n_out][S][S]
    const MetroPlacement* rec;    // [max_n]
    const int* rows;              // [n_rows]
    const int* starts;            // [n_persons + 1]
    const int* mirror;            // [n_out]
    const float* centres;         // [n_persons][n_out][3]: the caller's, or centres_out as the triangulation wrote it
    float* centres_out;           // [n_persons][n_out][3]
    float* points;                // [n_persons][n_out][3]
    float* cov;                   // [n_persons][n_out][9]
    float* stats;                 // [n_persons][n_out][2]
    int* info;                    // [n_persons][n_out][2]
    int n, n_rows, n_persons, n_out, S, G, V;
    double extent, pfloor, near, lrc, half_off;
};

// grid offset i of G along one axis
__host__ __device__ inline double vf_offset(int i, int G, double extent) { return -extent / 2.0 + (double)i * (extent / (double)(G - 1)); }

// ln max(p, floor) of one row's map at the projection of world point x; ln floor where the point lies behind (or nearer than
// near_mm to) the camera or projects outside the map.  Every test is written so that a NaN takes the floor.
__host__ __device__ inline double vf_row_logp(const VfRow& w, const double* x, int S, double lrc, double half_off, double near,
                                              double pfloor, double ln_floor) {
    const double d[3] = {x[0] - w.o[0], x[1] - w.o[1], x[2] - w.o[2]};
    const double cx = (w.r[0] * d[0] + w.r[3] * d[1]) + w.r[6] * d[2];          // R^T d
    const double cy = (w.r[1] * d[0] + w.r[4] * d[1]) + w.r[7] * d[2];
    const double cz = (w.r[2] * d[0] + w.r[5] * d[1]) + w.r[8] * d[2];
    if (!(cz > near)) return ln_floor;
    const double nx = cx / cz, ny = cy / cz;
    const double u = (w.k[0] * nx + w.k[1] * ny) + w.k[2], v = (w.k[3] * nx + w.k[4] * ny) + w.k[5];
    const double last = (double)(S - 1);
    const double fx = ((u - half_off) / lrc) * last, fy = ((v - half_off) / lrc) * last;
    if (!(fx >= 0.0 && fx <= last && fy >= 0.0 && fy <= last)) return ln_floor;
    int x0 = (int)fx, y0 = (int)fy;                                              // fx, fy >= 0: truncation is the floor
    if (x0 > S - 2) x0 = S - 2;
    if (y0 > S - 2) y0 = S - 2;
    const double tx = fx - (double)x0, ty = fy - (double)y0;
    const float* m = w.map + (size_t)y0 * S + x0;
    const double a = (double)m[0], b = (double)m[1], c = (double)m[S], e = (double)m[S + 1];
    const double top = a + tx * (b - a), bot = c + tx * (e - c);
    double p = top + ty * (bot - top);
    // a bilinear value lies between its cells; rounding may carry it an ulp past the largest one, and the agreement must not
    // come out above 0 for that
    if (p > (double)w.cmax) p = (double)w.cmax;
    return log(p > pfloor ? p : pfloor);
}

template <class Team>
__host__ __device__ inline void fusion_walk(const ViewFusionArgs& a, int item, char* lds, Team& team) {
    const int person = item / a.n_out, r = item - person * a.n_out;
    const int tid = team.tid, nt = team.nt;
    const int G = a.G, vol = G * G * G, cells = a.S * a.S;
    VfRow* row = reinterpret_cast<VfRow*>(lds + VF_LDS_HEAD);
    double* E = reinterpret_cast<double*>(lds + VF_LDS_ROWS);
    float* points = a.points + (size_t)item * 3;
    float* cov = a.cov + (size_t)item * 9;
    float* stats = a.stats + (size_t)item * 2;
    int* info = a.info + (size_t)item * 2;
    const float nan = __builtin_nanf("");

    const float cf[3] = {a.centres[(size_t)item * 3], a.centres[(size_t)item * 3 + 1], a.centres[(size_t)item * 3 + 2]};
    if (a.centres != a.centres_out && tid == 0)
        for (int t = 0; t < 3; ++t) a.centres_out[(size_t)item * 3 + t] = cf[t];
    const double ctr[3] = {(double)cf[0], (double)cf[1], (double)cf[2]};
    int first = a.starts[person], last = a.starts[person + 1];
    if (first < 0) first = 0;
    if (last > a.n_rows) last = a.n_rows;
    const bool centred = __builtin_isfinite(ctr[0]) && __builtin_isfinite(ctr[1]) && __builtin_isfinite(ctr[2]);
    const double ln_floor = log(a.pfloor);

    int n_used = 0;
    double lsum = 0.0;                       // sum over the used rows of ln max(largest cell, floor), in row order as E is summed
    for (int k0 = first; centred && k0 < last; k0 += VF_CHUNK) {
        const int cnt = last - k0 < VF_CHUNK ? last - k0 : VF_CHUNK;
        // ---- the chunk's row records ----
        for (int t = tid; t < cnt; t += nt) {
            VfRow w;
            const int i = a.rows[k0 + t];
            w.used = 0; w.map = nullptr; w.cmax = 0.f;
            for (int e = 0; e < 6; ++e) w.k[e] = 0.0;
            for (int e = 0; e < 9; ++e) w.r[e] = 0.0;
            for (int e = 0; e < 3; ++e) w.o[e] = 0.0;
            if (i >= 0 && i < a.n) {
                const MetroPlacement& rec = a.rec[i];
                bool ok = true;
                double ki[9], k[9];
                for (int e = 0; e < 9; ++e) {
                    ki[e] = (double)rec.inv_intrinsics[e];
                    w.r[e] = (double)rec.rot_to_world[e];
                    ok = ok && __builtin_isfinite(ki[e]) && __builtin_isfinite(w.r[e]);
                }
                for (int e = 0; e < 3; ++e) {
                    w.o[e] = (double)rec.cam_loc[e];
                    ok = ok && __builtin_isfinite(w.o[e]);
                }
                const int src = mirrored(rec.rot_to_world) ? a.mirror[r] : r;
                ok = ok && src >= 0 && src < a.n_out;              // a mirror table that points outside the skeleton
                if (ok) {
                    inv3(ki, k);
                    for (int e = 0; e < 6; ++e) w.k[e] = k[e];
                    w.map = a.xy + ((size_t)i * a.n_out + src) * cells;
                    w.used = 1;
                }
            }
            row[t] = w;
        }
        team.sync();
        // ---- each map's largest cell; +Inf where a cell is not finite ----
        float mx[VF_CHUNK];
#pragma unroll
        for (int k = 0; k < VF_CHUNK; ++k) {
            mx[k] = -INFINITY;
            if (k < cnt && row[k].used) {
                const float* m = row[k].map;
                for (int c = tid; c < cells; c += nt) {
                    const float v = m[c];
                    mx[k] = __builtin_isfinite(v) ? (v > mx[k] ? v : mx[k]) : INFINITY;
                }
            }
        }
        team.template maxes<VF_CHUNK>(mx);
#pragma unroll
        for (int k = 0; k < VF_CHUNK; ++k)
            if (k < cnt && tid == k % nt) row[k].cmax = mx[k];
        team.sync();
        // ---- the chunk's rows into E ----
        for (int k = 0; k < cnt; ++k) {
            if (!(row[k].used && row[k].cmax < INFINITY)) continue;
            const double top = (double)row[k].cmax;
            lsum += log(top > a.pfloor ? top : a.pfloor);
            ++n_used;
        }
        for (int v = tid; v < vol; v += nt) {
            const int ia = v / (G * G), rem = v - ia * G * G, ib = rem / G, ic = rem - ib * G;
            const double x[3] = {ctr[0] + vf_offset(ia, G, a.extent), ctr[1] + vf_offset(ib, G, a.extent), ctr[2] + vf_offset(ic, G, a.extent)};
            double acc = k0 == first ? 0.0 : E[v];
            for (int k = 0; k < cnt; ++k)
                if (row[k].used && row[k].cmax < INFINITY) acc += vf_row_logp(row[k], x, a.S, a.lrc, a.half_off, a.near, a.pfloor, ln_floor);
            E[v] = acc;
        }
        team.sync();                         // the records are written again
    }
    if (n_used == 0) {                       // a centre that is not finite, an empty group, no usable row
        if (tid == 0) {
            for (int t = 0; t < 3; ++t) points[t] = nan;
            for (int t = 0; t < 9; ++t) cov[t] = nan;
            stats[0] = stats[1] = nan;
            info[0] = 0; info[1] = 0;
        }
        return;
    }

    // ---- 1: E = sum / V, its maximum at the lowest index ----
    const double views = (double)a.V;
    double best = -INFINITY;
    int best_v = 0x7fffffff;
    for (int v = tid; v < vol; v += nt) {
        const double e = E[v] / views;
        E[v] = e;
        if (e > best) { best = e; best_v = v; }
    }
    team.argmax(best, best_v);
    const double M = best;

    // ---- 2: the normaliser and the first moments of the offsets from the centre ----
    double s1[4] = {0, 0, 0, 0};
    for (int v = tid; v < vol; v += nt) {
        const int ia = v / (G * G), rem = v - ia * G * G, ib = rem / G, ic = rem - ib * G;
        const double e = exp(E[v] - M);
        s1[0] += e;
        s1[1] += e * vf_offset(ia, G, a.extent); s1[2] += e * vf_offset(ib, G, a.extent); s1[3] += e * vf_offset(ic, G, a.extent);
    }
    team.template sums<4>(s1);
    const double inv = 1.0 / s1[0];
    const double m0 = s1[1] * inv, m1 = s1[2] * inv, m2 = s1[3] * inv;

    // ---- 3: the central second moments ----
    double s2[6] = {0, 0, 0, 0, 0, 0};
    for (int v = tid; v < vol; v += nt) {
        const int ia = v / (G * G), rem = v - ia * G * G, ib = rem / G, ic = rem - ib * G;
        const double w = exp(E[v] - M) * inv;
        const double ex = vf_offset(ia, G, a.extent) - m0, ey = vf_offset(ib, G, a.extent) - m1, ez = vf_offset(ic, G, a.extent) - m2;
        s2[0] += w * ex * ex; s2[1] += w * ey * ey; s2[2] += w * ez * ez;
        s2[3] += w * ex * ey; s2[4] += w * ex * ez; s2[5] += w * ey * ez;
    }
    team.template sums<6>(s2);
    if (tid == 0) {
        points[0] = (float)(ctr[0] + m0); points[1] = (float)(ctr[1] + m1); points[2] = (float)(ctr[2] + m2);
        const float c6[6] = {(float)s2[0], (float)s2[1], (float)s2[2], (float)s2[3], (float)s2[4], (float)s2[5]};
        cov[0] = c6[0]; cov[1] = c6[3]; cov[2] = c6[4];
        cov[3] = c6[3]; cov[4] = c6[1]; cov[5] = c6[5];
        cov[6] = c6[4]; cov[7] = c6[5]; cov[8] = c6[2];
        stats[0] = (float)inv;                                     // exp(M - M) / sum
        stats[1] = (float)(M - lsum / views);
        const int ia = best_v / (G * G), rem = best_v - ia * G * G, ib = rem / G, ic = rem - ib * G;
        info[0] = n_used;
        info[1] = (ia == 0 || ia == G - 1 || ib == 0 || ib == G - 1 || ic == 0 || ic == G - 1) ? 1 : 0;
    }
}

// The kernel's team: the workgroup, by the scheme of heat_posterior.hip's.  A 64-lane __shfl_xor ladder per value (every lane
// ends with the same bits: each step adds or compares the same two values in both lanes), one record per wave and value
// through LDS, folded in wave order by every thread; a second barrier, so that the records can be written again.
struct FusionWorkgroup {
    char* rec;                                       // LDS, VF_LDS_HEAD bytes
    const int tid;
    static constexpr int nt = VF_THREADS, n_groups = VF_THREADS / 64;
    const int group, lane;

    __device__ void sync() const { __syncthreads(); }
    template <int N, typename T>
    __device__ void maxes(T (&x)[N]) const {
        static_assert(n_groups * N * sizeof(T) <= (size_t)VF_LDS_HEAD, "wave records");
        T* w = reinterpret_cast<T*>(rec);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            for (int off = 32; off > 0; off >>= 1) {
                const T o = __shfl_xor(x[i], off);
                x[i] = o > x[i] ? o : x[i];
            }
            if (lane == 0) w[group * N + i] = x[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < N; ++i) {
            x[i] = w[i];
            for (int g = 1; g < n_groups; ++g) x[i] = w[g * N + i] > x[i] ? w[g * N + i] : x[i];
        }
        __syncthreads();
    }
    template <int N, typename T>
    __device__ void sums(T (&x)[N]) const {
        static_assert(n_groups * N * sizeof(T) <= (size_t)VF_LDS_HEAD, "wave records");
        T* w = reinterpret_cast<T*>(rec);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            for (int off = 32; off > 0; off >>= 1) x[i] += __shfl_xor(x[i], off);
            if (lane == 0) w[group * N + i] = x[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < N; ++i) {
            x[i] = w[i];
            for (int g = 1; g < n_groups; ++g) x[i] += w[g * N + i];
        }
        __syncthreads();
    }
    // the largest value, at the lowest index among equals
    __device__ void argmax(double& v, int& idx) const {
        double* wv = reinterpret_cast<double*>(rec);
        int* wi = reinterpret_cast<int*>(rec + n_groups * sizeof(double));
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(v, off);
            const int oi = __shfl_xor(idx, off);
            if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
        }
        if (lane == 0) { wv[group] = v; wi[group] = idx; }
        __syncthreads();
        v = wv[0]; idx = wi[0];
        for (int g = 1; g < n_groups; ++g)
            if (wv[g] > v || (wv[g] == v && wi[g] < idx)) { v = wv[g]; idx = wi[g]; }
        __syncthreads();
    }
};

__global__ __launch_bounds__(VF_THREADS) void view_fusion_kernel(ViewFusionArgs a) {
    __shared__ __attribute__((aligned(16))) char vf_smem[VF_LDS_BYTES];
    FusionWorkgroup team = {vf_smem, (int)threadIdx.x, (int)threadIdx.x >> 6, (int)threadIdx.x & 63};
    fusion_walk(a, blockIdx.x, vf_smem, team);
}

ViewFusionArgs make_view_fusion_args(const float* xy, const MetroPlacement* rec, const int* rows, int n_rows, const int* starts,
                                     int n_persons, const int* mirror, const float* centres, const MetroViewFusion& params, int n,
                                     const MetroSpec& spec, float* points, float* cov, float* stats, int* info, float* centres_out) {
    ViewFusionArgs a;
    a.xy = xy; a.rec = rec; a.rows = rows; a.starts = starts; a.mirror = mirror;
    a.centres = centres != nullptr ? centres : centres_out; a.centres_out = centres_out;
    a.points = points; a.cov = cov; a.stats = stats; a.info = info;
    a.n = n; a.n_rows = n_rows; a.n_persons = n_persons; a.n_out = spec.n_joints_out;
    a.S = spec.stride > 0 ? spec.proc_side / spec.stride : 0; a.G = params.grid; a.V = params.n_views;
    a.extent = params.extent_mm; a.pfloor = params.floor; a.near = params.near_mm;
    const HeadPixelScale px = head_pixel_scale(spec);
    a.lrc = (double)px.lrc; a.half_off = (double)px.half_off;
    return a;
}

int launch_view_fusion(const float* xy, const MetroPlacement* rec, const int* rows, int n_rows, const int* starts, int n_persons,
                       const int* mirror, const float* centres, const MetroViewFusion& params, int n, const MetroSpec& spec,
                       float* points, float* cov, float* stats, int* info, float* centres_out, hipStream_t stream) {
    const ViewFusionArgs a = make_view_fusion_args(xy, rec, rows, n_rows, starts, n_persons, mirror, centres, params, n, spec, points,
                                                   cov, stats, info, centres_out);
    if (a.S < 2 || a.G < 2 || a.G > VF_MAX_GRID || a.V < 1 || a.n_out < 1 || a.n_out > METRO_MAX_JOINTS || n_persons < 0 ||
        (int64_t)n_persons * a.n_out > (int64_t)0x7fffffff) {
        set_error("view_fusion: unsupported call (a %d x %d map, grid %d, %d views, %d output joints, %d persons)", a.S, a.S, a.G, a.V,
                  a.n_out, n_persons);
        return METRO_ERR_UNSUPPORTED;
    }
    if (n_persons == 0) return METRO_OK;
    if (note_kernel("view_fusion<g%d>", a.G)) return METRO_OK;
    hipLaunchKernelGGL(view_fusion_kernel, dim3(n_persons * a.n_out), dim3(VF_THREADS), 0, stream, a);
    return launch_status("view_fusion");
}

}  // namespace metro
