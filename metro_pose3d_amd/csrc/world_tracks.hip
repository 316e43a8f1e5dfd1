// The time step of every person metro_cluster_views found, and the persons sorted into the time-step CSR
// metro_associate_tracks reads, built on the device between the triangulation and the association launch (metro_person_steps,
// include/metro_hip.h).  Nothing in the reference to restate: one example is one image of one camera.
// ONE workgroup of PERSON_STEPS_THREADS = METRO_MATCH_MAX_BOXES threads, thread p = person p.
//   1. step[p]: the smallest box_step[row / n_views] over the crop rows rows[starts[p] : starts[p + 1]] of the person's group
//      (clusters gated by step hold one value; ungated ones take the earliest).  -1 for p >= n_persons[0] and for an empty
//      group.  A row outside [0, n_boxes n_views) and a step outside [0, n_steps) are skipped, not read; starts is clamped to
//      [0, n_rows].  person_times[p] = step_times[step[p]], NaN where step[p] is -1.
//   2. rank: person p with a step stands behind the persons q with (step[q], q) < (step[p], p); step_rows[rank] = p, the
//      entries from the number of persons with a step on are -1.  step_starts[s] = the persons with a step below s, s = 0 .. S.
// At n <= 128 the O(n^2) count is a few hundred LDS reads per thread: no prefix sum is needed.
#include "metro_common.h"

namespace metro {

constexpr int PERSON_STEPS_THREADS = METRO_MATCH_MAX_BOXES;

struct PersonStepsArgs {
    const int* rows;                  // [n_rows] crop rows of the persons' groups (metro_cluster_views)
    const int* starts;                // [n + 1]
    const int* n_persons;             // [1]
    const int* box_step;              // [n_boxes]
    const double* step_times;         // [n_steps] ascending
    int* person_step;                 // [n]
    double* person_times;             // [n]
    int* step_rows;                   // [n]
    int* step_starts;                 // [n_steps + 1]
    int n, n_rows, n_views, n_boxes, n_steps;
};

// the step of person p, into step[p] (the workgroup's copy) and the two per-person outputs
__host__ __device__ inline void person_steps_assign(const PersonStepsArgs& a, int* step, int p) {
    int best = -1;
    if (p < a.n_persons[0]) {
        int first = a.starts[p], last = a.starts[p + 1];
        if (first < 0) first = 0;
        if (last > a.n_rows) last = a.n_rows;
        for (int k = first; k < last; ++k) {
            const int row = a.rows[k];
            if (row < 0 || row / a.n_views >= a.n_boxes) continue;
            const int s = a.box_step[row / a.n_views];
            if ((unsigned)s >= (unsigned)a.n_steps) continue;
            if (best < 0 || s < best) best = s;
        }
    }
    step[p] = best;
    a.person_step[p] = best;
    a.person_times[p] = best >= 0 ? a.step_times[best] : __builtin_nan("");
}

// person p's place among the persons sorted by (step, person)
__host__ __device__ inline void person_steps_rank(const PersonStepsArgs& a, const int* step, int p) {
    int rank = 0, total = 0;
    for (int q = 0; q < a.n; ++q) {
        total += step[q] >= 0;
        rank += step[q] >= 0 && (step[q] < step[p] || (step[q] == step[p] && q < p));
    }
    if (step[p] >= 0) a.step_rows[rank] = p;
    if (p >= total) a.step_rows[p] = -1;
}

// thread tid of nt covers the offsets tid, tid + nt, ...
__host__ __device__ inline void person_steps_starts(const PersonStepsArgs& a, const int* step, int tid, int nt) {
    for (int s = tid; s <= a.n_steps; s += nt) {
        int below = 0;
        for (int q = 0; q < a.n; ++q) below += step[q] >= 0 && step[q] < s;
        a.step_starts[s] = below;
    }
}

__global__ __launch_bounds__(PERSON_STEPS_THREADS) void person_steps_kernel(PersonStepsArgs a) {
    __shared__ int step[PERSON_STEPS_THREADS];
    const int p = threadIdx.x;
    if (p < a.n) person_steps_assign(a, step, p);
    __syncthreads();
    if (p < a.n) person_steps_rank(a, step, p);
    person_steps_starts(a, step, p, PERSON_STEPS_THREADS);
}

int launch_person_steps(const int* rows, int n_rows, const int* starts, const int* n_persons, int n, int n_views, const int* box_step,
                        int n_boxes, const double* step_times, int n_steps, int* person_step, double* person_times, int* step_rows,
                        int* step_starts, hipStream_t stream) {
    if (note_kernel("person_steps")) return METRO_OK;
    PersonStepsArgs a;
    a.rows = rows; a.starts = starts; a.n_persons = n_persons; a.box_step = box_step; a.step_times = step_times;
    a.person_step = person_step; a.person_times = person_times; a.step_rows = step_rows; a.step_starts = step_starts;
    a.n = n; a.n_rows = n_rows; a.n_views = n_views; a.n_boxes = n_boxes; a.n_steps = n_steps;
    hipLaunchKernelGGL(person_steps_kernel, dim3(1), dim3(PERSON_STEPS_THREADS), 0, stream, a);
    return launch_status("person_steps");
}

// ---- the same from the persons' labels alone (metro_person_steps_labels): a person with ONE box gets a step too ----
// metro_cluster_views leaves the group of a person seen by one camera empty, so person_steps_kernel gives it no step.  Here
// thread p walks person_index [n_boxes] itself: step[p] = the smallest valid box_step[b] over the boxes b with
// person_index[b] == p (for a person with several boxes the value person_steps_assign finds in its group), and
// single_box[p] = that box if the person has exactly one box and it has a valid step, else -1 (-1 also for p >= n_persons[0]).  A label outside [0, n) belongs to
// nobody; a step outside [0, n_steps) is skipped.  Rank and starts are person_steps_kernel's own functions.
struct PersonLabelsArgs : PersonStepsArgs {
    const int* person_index;          // [n_boxes] the person of every box (metro_cluster_views)
    int* single_box;                  // [n]
};

__host__ __device__ inline void person_labels_assign(const PersonLabelsArgs& a, int* step, int p) {
    int best = -1, boxes = 0, box = -1;
    if (p < a.n_persons[0]) {
        for (int b = 0; b < a.n_boxes; ++b) {
            if (a.person_index[b] != p) continue;
            ++boxes;
            const int s = a.box_step[b];
            if ((unsigned)s >= (unsigned)a.n_steps) continue;
            if (best < 0 || s < best) best = s;
            box = b;
        }
    }
    step[p] = best;
    a.person_step[p] = best;
    a.person_times[p] = best >= 0 ? a.step_times[best] : __builtin_nan("");
    a.single_box[p] = boxes == 1 && best >= 0 ? box : -1;
}

__global__ __launch_bounds__(PERSON_STEPS_THREADS) void person_steps_labels_kernel(PersonLabelsArgs a) {
    __shared__ int step[PERSON_STEPS_THREADS];
    const int p = threadIdx.x;
    if (p < a.n) person_labels_assign(a, step, p);
    __syncthreads();
    if (p < a.n) person_steps_rank(a, step, p);
    person_steps_starts(a, step, p, PERSON_STEPS_THREADS);
}

int launch_person_steps_labels(const int* person_index, const int* n_persons, int n, const int* box_step, int n_boxes,
                               const double* step_times, int n_steps, int* person_step, double* person_times, int* step_rows,
                               int* step_starts, int* single_box, hipStream_t stream) {
    if (note_kernel("person_steps_labels")) return METRO_OK;
    PersonLabelsArgs a;
    a.rows = nullptr; a.starts = nullptr; a.n_persons = n_persons; a.box_step = box_step; a.step_times = step_times;
    a.person_step = person_step; a.person_times = person_times; a.step_rows = step_rows; a.step_starts = step_starts;
    a.n = n; a.n_rows = 0; a.n_views = 1; a.n_boxes = n_boxes; a.n_steps = n_steps;
    a.person_index = person_index; a.single_box = single_box;
    hipLaunchKernelGGL(person_steps_labels_kernel, dim3(1), dim3(PERSON_STEPS_THREADS), 0, stream, a);
    return launch_status("person_steps_labels");
}

}  // namespace metro
