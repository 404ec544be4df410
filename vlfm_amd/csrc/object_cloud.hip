// object_cloud.hip -- gfx950 kernels for vlfm.mapping.ObjectPointCloudMap._extract_object_cloud
// (reference: /root/reference/vlfm/mapping/object_point_cloud_map.py:150-170, :186-212).
//
//   mask_*_batch_kernel       cv2.erode(mask * 255, None, iterations=k): 3x3 minimum, image border does not erode
//                             (morphologyDefaultBorderValue) -- on a bit-packed mask, one AND of nine shifted words per word;
//                             then per-row popcounts and their scan: the row offsets of the masked pixels in np.where order
//   cloud_expand_batch_kernel valid_depth (0 -> 1), scale, get_point_cloud (geometry_utils.py:216-236) -> f64 points (z, -x, -y).
//                             One thread per OUTPUT slot finds its pixel by rank (binary search in the row offsets, popcount walk
//                             within the row), so the 5000-point subsample is taken while expanding and device memory is bounded
//                             by the number of points kept, not by the mask area
//   dbscan_*_batch_kernel     open3d PointCloud.cluster_dbscan(eps, min_points) [ext] for n <= ~5000 points, restated for a
//                             data-parallel machine: eps-adjacency as an n x n bit matrix (64 columns per word: a wavefront
//                             ballot), core = degree >= min_points (the point itself counts), clusters = connected components
//                             of the core-core graph labelled in order of their smallest core index (the order in which the
//                             sequential scan seeds them), border points join the lowest-labelled neighbouring cluster (the
//                             first one to reach them), everything else is noise; then the largest cluster (first maximum) in
//                             original point order (object_point_cloud_map.py:186-212).
// Latency-bound integer/f64 work on a few thousand points; no MFMA.
//
// Every kernel takes ALL detections of a step at once (grid.y = job, or one workgroup per job); a single detection is a batch of one.
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vlfm_amd.h"
#include "profile.h"
#include "status.h"

namespace vlfm {

// ------------------------------------------------------------------------------------------------ mask -> bits, erosion
// one eroded word of a packed plane: the AND of the nine shifted neighbours
__device__ __forceinline__ unsigned erode_word(const unsigned* __restrict__ src, int y, int w, int H, int W, int hw) {
    const unsigned tail = (W & 31) && w == hw - 1 ? ~((1u << (W & 31)) - 1u) : 0u;  // columns >= W count as set
    unsigned acc = 0xFFFFFFFFu;
    for (int dy = -1; dy <= 1; dy++) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;  // rows outside the image count as set
        const unsigned* row = src + (size_t)yy * hw;
        const unsigned m = row[w] | tail;
        const unsigned left = w > 0 ? row[w - 1] >> 31 : 1u;                                   // column -1 counts as set
        const unsigned right = w + 1 < hw ? (row[w + 1] | ((W & 31) && w + 1 == hw - 1 ? ~((1u << (W & 31)) - 1u) : 0u)) & 1u : 1u;
        acc &= m & ((m << 1) | left) & ((m >> 1) | (right << 31));
    }
    return acc & ~tail;
}

// grid.y = job.  The packed plane of every job, and the OR of its rows (which columns the UN-eroded mask occupies: the x-extent
// of cv2.boundingRect that too_offset asks for).  col_bits [jobs][hw] starts zeroed.
__global__ __launch_bounds__(256) void mask_pack_batch_kernel(const unsigned char* __restrict__ masks, int H, int W, int hw,
                                                              unsigned* __restrict__ bits, unsigned* __restrict__ col_bits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, job = blockIdx.y;
    if (i >= H * hw) return;
    const int y = i / hw, w = i - y * hw;
    const unsigned char* row = masks + ((size_t)job * H + y) * W;
    unsigned v = 0u;
    for (int b = 0; b < 32; b++) {
        const int x = w * 32 + b;
        if (x < W && row[x] != 0) v |= 1u << b;
    }
    bits[(size_t)job * H * hw + i] = v;
    if (v) atomicOr(&col_bits[(size_t)job * hw + w], v);
}

// grid.y = job; iteration k of the longest erosion of the batch.  A job that asked for k or fewer iterations carries its plane along.
__global__ __launch_bounds__(256) void mask_erode_batch_kernel(const unsigned* __restrict__ src, int H, int W, int hw,
                                                               const int* __restrict__ iterations, int k,
                                                               unsigned* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, job = blockIdx.y;
    if (i >= H * hw) return;
    const size_t plane = (size_t)job * H * hw;
    const int y = i / hw, w = i - y * hw;
    dst[plane + i] = iterations[job] > k ? erode_word(src + plane, y, w, H, W, hw) : src[plane + i];
}

// One workgroup per job: row offsets of the ordered expansion (kept in scratch for the expansion kernel), the point count and the
// first / last occupied column of the un-eroded mask (-1, -1 = empty).  stats [jobs][4] = (count, first column, last column, 0).
__global__ __launch_bounds__(1024) void mask_stats_batch_kernel(const unsigned* __restrict__ bits, const unsigned* __restrict__ col_bits,
                                                                int H, int hw, int* __restrict__ row_off_all,
                                                                int* __restrict__ stats) {
    extern __shared__ int row_off[];  // [H + 1]
    const int tid = threadIdx.x, nth = blockDim.x, job = blockIdx.x;
    const unsigned* plane = bits + (size_t)job * H * hw;
    for (int y = tid; y < H; y += nth) {
        int c = 0;
        for (int w = 0; w < hw; w++) c += __popc(plane[(size_t)y * hw + w]);
        row_off[y + 1] = c;
    }
    if (tid == 0) row_off[0] = 0;
    __syncthreads();
    if (tid == 0) {  // H <= a few thousand: a serial scan is microseconds
        for (int y = 0; y < H; y++) row_off[y + 1] += row_off[y];
        int first = -1, last = -1;
        for (int w = 0; w < hw; w++) {
            const unsigned v = col_bits[(size_t)job * hw + w];
            if (!v) continue;
            if (first < 0) first = w * 32 + __builtin_ctz(v);
            last = w * 32 + 31 - __builtin_clz(v);
        }
        stats[job * 4 + 0] = row_off[H];
        stats[job * 4 + 1] = first;
        stats[job * 4 + 2] = last;
        stats[job * 4 + 3] = 0;
    }
    __syncthreads();
    for (int y = tid; y <= H; y += nth) row_off_all[(size_t)job * (H + 1) + y] = row_off[y];
}

// ------------------------------------------------------------------------------------------------ masked unprojection
// valid_depth (0 -> 1), scale, get_point_cloud for pixel (u, y): the f64 point (z, -x, -y)
__device__ __forceinline__ void unproject_pixel(float d, int u, int y, int H, int W, float scale, float offset, double fx, double fy,
                                                double* __restrict__ out) {
    if (d == 0.0f) d = 1.0f;                                   // holes are "far" (:160-161)
    const float z = __fadd_rn(__fmul_rn(d, scale), offset);    // f32 (:162)
    const double zd = (double)z;
    const double xc = __ddiv_rn(__dmul_rn((double)(u - W / 2), zd), fx);   // geometry_utils.py:230-232
    const double yc = __ddiv_rn(__dmul_rn((double)(y - H / 2), zd), fy);
    out[0] = zd;
    out[1] = -xc;
    out[2] = -yc;
}

// grid.y = entry of `jobs`; one thread per OUTPUT point.  jobs [n][6] = (stage-1 job, depth frame, points to write, first output
// point, first entry of `ranks` or -1, 0).  Output slot s holds the masked pixel of rank ranks[first + s] (np.where order), or of
// rank s without a rank list: the row by binary search in the row offsets, the column by a popcount walk along the row.
__global__ __launch_bounds__(256) void cloud_expand_batch_kernel(const float* __restrict__ depth, int frames, const unsigned* __restrict__ bits,
                                                                 const int* __restrict__ row_off_all, int scratch_jobs, int H, int W,
                                                                 int hw, float scale, float offset, double fx, double fy,
                                                                 const int* __restrict__ jobs, const int* __restrict__ ranks,
                                                                 int n_ranks, double* __restrict__ points, int capacity) {
    const int* jd = jobs + (size_t)blockIdx.y * 6;
    const int job = jd[0], frame = jd[1], n_out = jd[2], first = jd[3], rank0 = jd[4];
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_out || job < 0 || job >= scratch_jobs || frame < 0 || frame >= frames || first < 0 || first > capacity - n_out) return;
    const int* row_off = row_off_all + (size_t)job * (H + 1);
    if (rank0 >= 0 && rank0 > n_ranks - n_out) return;
    const int r = rank0 >= 0 ? ranks[rank0 + s] : s;
    if (r < 0 || r >= row_off[H]) return;
    int lo = 0, hi = H - 1;                       // the last row with row_off[y] <= r (empty rows repeat their offset)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (row_off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    const int y = lo;
    const unsigned* row = bits + ((size_t)job * H + y) * hw;
    int k = r - row_off[y];                       // the k-th set bit of the row
    for (int w = 0; w < hw; w++) {
        unsigned v = row[w];
        const int pc = __popc(v);
        if (k >= pc) { k -= pc; continue; }
        for (; k > 0; k--) v &= v - 1;
        const int u = w * 32 + __builtin_ctz(v);
        unproject_pixel(depth[((size_t)frame * H + y) * W + u], u, y, H, W, scale, offset, fx, fy, points + (size_t)(first + s) * 3);
        return;
    }
}

// ------------------------------------------------------------------------------------------------ DBSCAN
// adjacency: word (i, cb) bit j = |p_i - p_(64 cb + j)|^2 < eps^2 (strict: nanoflann's radius search); one wavefront per
// (row, column block): lane j tests point 64 cb + j, the ballot is the word.
__device__ __forceinline__ void dbscan_adjacency_row(const double* __restrict__ pts, int n, double eps2,
                                                     unsigned long long* __restrict__ adj, int cb_count, int* __restrict__ degree) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (i >= n) return;
    const double xi = pts[(size_t)i * 3], yi = pts[(size_t)i * 3 + 1], zi = pts[(size_t)i * 3 + 2];
    int deg = 0;
    for (int cb = 0; cb < cb_count; cb++) {
        const int j = cb * 64 + lane;
        bool near = false;
        if (j < n) {
            const double dx = pts[(size_t)j * 3] - xi, dy = pts[(size_t)j * 3 + 1] - yi, dz = pts[(size_t)j * 3 + 2] - zi;
            near = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)) < eps2;
        }
        const unsigned long long word = __ballot(near);
        if (lane == 0) adj[(size_t)i * cb_count + cb] = word;
        deg += __popcll(word);
    }
    if (lane == 0) degree[i] = deg;
}

// Per-job scratch of the DBSCAN: adjacency words, then degree, sizes, label, keep ([n] i32 each) -- the layout include/vlfm_amd.h states.
struct DbscanJob {
    const double* pts;
    unsigned long long* adj;
    int *degree, *sizes, *label, *keep;
    int n, cb, first;
};
__device__ __forceinline__ size_t dbscan_batch_job_bytes(int n) {
    const size_t cb = ((size_t)n + 63) / 64;
    return ((size_t)n * cb * 8 + (size_t)4 * n * sizeof(int) + 255) & ~(size_t)255;
}
// jobs [n_jobs][3] i64 = (points, first point, byte offset of the job's scratch).  false = nothing to do (n == 0) or a descriptor
// that does not fit its buffers (never produced by the host side; refused here so that no thread writes out of bounds).
__device__ __forceinline__ bool dbscan_batch_job(const long long* __restrict__ jobs, int j, const double* __restrict__ points,
                                                 int capacity, void* scratch, size_t scratch_bytes, int max_n, DbscanJob& out) {
    const long long n = jobs[(size_t)j * 3], first = jobs[(size_t)j * 3 + 1], off = jobs[(size_t)j * 3 + 2];
    if (n <= 0 || n > max_n || n > 8192 || first < 0 || first + n > capacity || off < 0 || (off & 255)) return false;
    if ((unsigned long long)off + dbscan_batch_job_bytes((int)n) > scratch_bytes) return false;
    out.n = (int)n;
    out.cb = ((int)n + 63) / 64;
    out.first = (int)first;
    out.pts = points + (size_t)first * 3;
    out.adj = (unsigned long long*)((unsigned char*)scratch + off);
    out.degree = (int*)(out.adj + (size_t)out.n * out.cb);
    out.sizes = out.degree + n;
    out.label = out.sizes + n;
    out.keep = out.label + n;
    return true;
}

__global__ __launch_bounds__(256) void dbscan_adjacency_batch_kernel(const double* __restrict__ points, int capacity,
                                                                     const long long* __restrict__ jobs, int max_n, double eps2,
                                                                     void* scratch, size_t scratch_bytes) {
    DbscanJob J;
    if (!dbscan_batch_job(jobs, blockIdx.y, points, capacity, scratch, scratch_bytes, max_n, J)) return;
    dbscan_adjacency_row(J.pts, J.n, eps2, J.adj, J.cb, J.degree);
}

// One workgroup: connected components of the core graph by BIT-PARALLEL breadth-first search (round 4; before: min-label propagation
// that enumerated every neighbour of every core point once per sweep -- 5000 points of one dense object blob have ~1000 neighbours each,
// and with the serial size / compaction loops of one lane a call took 20-35 ms, which made the object-map stage THE cost of the
// batched full step).  The eps-adjacency is already a bit matrix; a search level is "OR the adjacency rows of the frontier": every
// wavefront takes frontier nodes, its lanes OR the row's words (masked by the core set) into registers, and the wavefront's result
// goes to LDS once per level -- n x n / 64 word operations per component in total, no neighbour enumeration.  Components are seeded
// in ascending order of their smallest core index (the order in which the sequential scan of the reference's Open3D seeds them), so
// label = that index, as before.  Border points have fewer than min_points neighbours: enumerating those is cheap.  Cluster sizes,
// the first largest cluster and the ordered index list are parallel reductions / prefix sums.  n <= 8192.
constexpr int DB_WORDS = 128;    // 8192 / 64

__device__ __forceinline__ void dbscan_cluster_block(const unsigned long long* __restrict__ adj, const int* __restrict__ degree,
                                                     int n, int cb_count, int min_points, int* __restrict__ label,
                                                     int* __restrict__ sizes /* [n] scratch */, int* __restrict__ keep,
                                                     int* __restrict__ num_keep) {
    __shared__ unsigned long long core[DB_WORDS], unvis[DB_WORDS], comp[DB_WORDS], front[DB_WORDS], nxt[DB_WORDS];
    __shared__ int sh_root, sh_more, best_label, best_size;
    __shared__ int wprefix[DB_WORDS + 1];
    __shared__ unsigned long long red_key[16];
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, wave = tid >> 6, nwaves = nth >> 6;
    // ---- core set as a bit set; every label starts as noise
    for (int base = 0; base < cb_count * 64; base += nth) {
        const int i = base + tid;
        const bool is_core = i < n && degree[i] >= min_points;
        const unsigned long long w = __ballot(is_core);
        if (lane == 0 && (i >> 6) < cb_count) { core[i >> 6] = w; unvis[i >> 6] = w; }
        if (i < n) { label[i] = 0x7FFFFFFF; sizes[i] = 0; }
    }
    __syncthreads();
    for (;;) {
        // ---- next seed: the smallest core index not yet in a component
        if (wave == 0) {
            int first = 0x7FFFFFFF;
            for (int wd = lane; wd < cb_count; wd += 64)
                if (unvis[wd] && first == 0x7FFFFFFF) first = wd * 64 + __builtin_ctzll(unvis[wd]);
            for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off, 64));
            if (lane == 0) sh_root = first;
        }
        __syncthreads();
        const int root = sh_root;
        if (root == 0x7FFFFFFF) break;
        for (int wd = tid; wd < cb_count; wd += nth) {
            const unsigned long long b = wd == (root >> 6) ? (1ull << (root & 63)) : 0ull;
            comp[wd] = b; front[wd] = b; nxt[wd] = 0ull;
        }
        __syncthreads();
        // ---- breadth-first levels
        for (;;) {
            // lane l of a wavefront accumulates words l and l + 64 of the rows of the frontier nodes its wavefront takes
            unsigned long long a0 = 0ull, a1 = 0ull;
            for (int wd = wave; wd < cb_count; wd += nwaves) {
                unsigned long long f = front[wd];          // wave-uniform
                while (f) {
                    const int i = wd * 64 + __builtin_ctzll(f);
                    f &= f - 1;
                    const unsigned long long* row = adj + (size_t)i * cb_count;
                    if (lane < cb_count) a0 |= row[lane];
                    if (lane + 64 < cb_count) a1 |= row[lane + 64];
                }
            }
            if (lane < cb_count && a0) atomicOr(&nxt[lane], a0 & core[lane]);
            if (lane + 64 < cb_count && a1) atomicOr(&nxt[lane + 64], a1 & core[lane + 64]);
            if (tid == 0) sh_more = 0;
            __syncthreads();
            for (int wd = tid; wd < cb_count; wd += nth) {
                const unsigned long long fresh = nxt[wd] & ~comp[wd];
                comp[wd] |= fresh; front[wd] = fresh; nxt[wd] = 0ull;
                if (fresh) sh_more = 1;
            }
            __syncthreads();
            if (!sh_more) break;
            __syncthreads();
        }
        // ---- the component's label, and out of the unvisited set
        for (int i = tid; i < cb_count * 64; i += nth)
            if (i < n && ((comp[i >> 6] >> (i & 63)) & 1ull)) label[i] = root;
        for (int wd = tid; wd < cb_count; wd += nth) unvis[wd] &= ~comp[wd];
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    // ---- border points: the lowest-labelled neighbouring core cluster (clusters are seeded in order of their smallest core index, so
    // "lowest root index" == "first cluster to reach the point"); noise keeps INT_MAX.  Read core labels only: border points do not feed
    // each other (their own labels are written after the barrier)
    for (int i = tid; i < n; i += nth) {
        int best = 0x7FFFFFFF;
        if (degree[i] < min_points) {
            const unsigned long long* row = adj + (size_t)i * cb_count;
            for (int cb = 0; cb < cb_count; cb++) {
                unsigned long long w = row[cb] & core[cb];
                while (w) {
                    const int j = cb * 64 + __builtin_ctzll(w);
                    w &= w - 1;
                    best = min(best, label[j]);
                }
            }
        }
        sizes[i] = best;   // staged
    }
    __syncthreads();
    for (int i = tid; i < n; i += nth) if (degree[i] < min_points) label[i] = sizes[i];
    __syncthreads();
    for (int i = tid; i < n; i += nth) sizes[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += nth) if (label[i] != 0x7FFFFFFF) atomicAdd(&sizes[label[i]], 1);
    __syncthreads();
    // ---- np.argmax over clusters in label order (roots ascending == labels ascending): the FIRST maximum = largest size, then the
    // smallest root.  key = size << 32 | (0xFFFFFFFF - root): the maximum key wins
    unsigned long long key = 0ull;
    for (int r = tid; r < n; r += nth) {
        const int sz = sizes[r];
        if (sz > 0) { const unsigned long long k = ((unsigned long long)(unsigned)sz << 32) | (0xFFFFFFFFu - (unsigned)r); key = k > key ? k : key; }
    }
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(key, off, 64); key = o > key ? o : key; }
    if (lane == 0) red_key[wave] = key;
    __syncthreads();
    if (tid == 0) {
        unsigned long long k = 0ull;
        for (int w = 0; w < nwaves; w++) k = red_key[w] > k ? red_key[w] : k;
        best_size = (int)(k >> 32);
        best_label = k ? (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull)) : -1;
    }
    __syncthreads();
    if (best_label < 0) { if (tid == 0) *num_keep = 0; return; }
    // ---- ordered compaction (np.where order): membership bit set -> per-word prefix -> every member writes its own slot
    const int bl = best_label;
    for (int base = 0; base < cb_count * 64; base += nth) {
        const int i = base + tid;
        const unsigned long long w = __ballot(i < n && label[i] == bl);
        if (lane == 0 && (i >> 6) < cb_count) comp[i >> 6] = w;
    }
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        for (int wd = 0; wd < cb_count; wd++) { wprefix[wd] = c; c += __popcll(comp[wd]); }   // <= 128 LDS words
        wprefix[cb_count] = c;
        *num_keep = c;
    }
    __syncthreads();
    for (int i = tid; i < n; i += nth) {
        const unsigned long long w = comp[i >> 6];
        if ((w >> (i & 63)) & 1ull) keep[wprefix[i >> 6] + __popcll(w & ((1ull << (i & 63)) - 1ull))] = i;
    }
}

// One workgroup per job, each with its own n; then the points of the largest cluster, in order, at the job's own place in `kept`
// (the same offsets as `points`: a job keeps at most what it had).
__global__ __launch_bounds__(1024) void dbscan_cluster_batch_kernel(const double* __restrict__ points, int capacity,
                                                                    const long long* __restrict__ jobs, int max_n, int min_points,
                                                                    void* scratch, size_t scratch_bytes, double* __restrict__ kept,
                                                                    int* __restrict__ num_keep) {
    const int j = blockIdx.x;
    DbscanJob J;
    if (!dbscan_batch_job(jobs, j, points, capacity, scratch, scratch_bytes, max_n, J)) {
        if (threadIdx.x == 0) num_keep[j] = 0;
        return;
    }
    dbscan_cluster_block(J.adj, J.degree, J.n, J.cb, min_points, J.label, J.sizes, J.keep, num_keep + j);
    __syncthreads();   // keep[] and num_keep[j] were written by other lanes of this workgroup
    const int k = ((volatile int*)num_keep)[j];
    double* out = kept + (size_t)J.first * 3;
    for (int t = threadIdx.x; t < k * 3; t += blockDim.x) out[t] = J.pts[(size_t)J.keep[t / 3] * 3 + t % 3];
}

}  // namespace vlfm

using namespace vlfm;

// every kernel this file launches is counted (vlfm_object_cloud_launch_count): the count per call does not depend on the number of
// detections, and the tests hold it to that
static std::atomic<long long> g_launches{0};
#define OC_LAUNCH(...)           \
    do {                         \
        g_launches.fetch_add(1); \
        VLFM_KLAUNCH(__VA_ARGS__); \
    } while (0)

extern "C" long long vlfm_object_cloud_launch_count(void) { return g_launches.load(); }

// ------------------------------------------------------------------------------------------------ all detections of a step
extern "C" size_t vlfm_object_cloud_batch_scratch_bytes(int jobs, int height, int width) {
    if (jobs <= 0 || height <= 0 || width <= 0) return 0;
    const size_t hw = ((size_t)width + 31) / 32;
    return (size_t)jobs * (2 * (size_t)height * hw + hw + (size_t)height + 1) * sizeof(uint32_t);
}

extern "C" int vlfm_object_cloud_batch_stats(const uint8_t* d_masks, const int32_t* d_erosion, int jobs, int max_erosion, int height,
                                             int width, void* d_scratch, int32_t* d_stats, void* stream) {
    if (jobs == 0) return VLFM_OK;
    if (!d_masks || !d_erosion || !d_scratch || !d_stats || jobs < 0 || jobs > 65535 || height <= 0 || width <= 0 ||
        max_erosion < 0 || height > 8192)
        return fail(VLFM_ERR_INVALID, "object_cloud_batch_stats: bad argument (jobs <= 65535, height <= 8192)");
    const int hw = (width + 31) / 32, words = height * hw;
    if ((size_t)jobs * words > 0x7FFFFFFFu) return fail(VLFM_ERR_CAPACITY, "object_cloud_batch_stats: too many mask words for one call");
    unsigned* a = (unsigned*)d_scratch;                 // the final planes end up here whatever the parity of max_erosion
    unsigned* b = a + (size_t)jobs * words;
    unsigned* col_bits = b + (size_t)jobs * words;
    int* row_off = (int*)(col_bits + (size_t)jobs * hw);
    if (hipMemsetAsync(col_bits, 0, (size_t)jobs * hw * sizeof(unsigned), (hipStream_t)stream) != hipSuccess)
        return fail(VLFM_ERR_HIP, "object_cloud_batch_stats: memset failed");
    const dim3 grid((words + 255) / 256, jobs);
    unsigned *src = (max_erosion & 1) ? b : a, *dst = (max_erosion & 1) ? a : b;
    OC_LAUNCH(mask_pack_batch_kernel, grid, dim3(256), 0, stream, d_masks, height, width, hw, src, col_bits);
    for (int k = 0; k < max_erosion; k++) {
        OC_LAUNCH(mask_erode_batch_kernel, grid, dim3(256), 0, stream, (const unsigned*)src, height, width, hw, d_erosion, k, dst);
        unsigned* t = src; src = dst; dst = t;
    }
    VLFM_TIMED("mask_stats_batch_kernel", stream);
    OC_LAUNCH(mask_stats_batch_kernel, dim3(jobs), dim3(1024), (size_t)(height + 1) * sizeof(int), stream, (const unsigned*)a,
              (const unsigned*)col_bits, height, hw, row_off, d_stats);
    return check_launch("mask_stats_batch_kernel");
}

extern "C" int vlfm_object_cloud_batch_expand(const float* d_depth, int frames, int height, int width, double min_depth,
                                              double max_depth, double fx, double fy, const void* d_scratch, int scratch_jobs,
                                              const int32_t* d_jobs, int n_jobs, int max_points, const int32_t* d_ranks,
                                              int n_ranks, double* d_points, int capacity, void* stream) {
    if (n_jobs == 0 || max_points == 0) return VLFM_OK;
    if (!d_depth || !d_scratch || !d_jobs || !d_points || frames <= 0 || height <= 0 || width <= 0 || height > 8192 ||
        scratch_jobs <= 0 || n_jobs < 0 || n_jobs > 65535 || max_points < 0 || capacity <= 0 || n_ranks < 0 ||
        (n_ranks > 0 && !d_ranks))
        return fail(VLFM_ERR_INVALID, "object_cloud_batch_expand: bad argument");
    const int hw = (width + 31) / 32;
    const size_t words = (size_t)height * hw;
    const unsigned* bits = (const unsigned*)d_scratch;
    const int* row_off = (const int*)(bits + (size_t)scratch_jobs * (2 * words + hw));
    VLFM_TIMED("cloud_expand_batch_kernel", stream);
    OC_LAUNCH(cloud_expand_batch_kernel, dim3((max_points + 255) / 256, n_jobs), dim3(256), 0, stream, d_depth, frames, bits, row_off,
              scratch_jobs, height, width, hw, (float)(max_depth - min_depth), (float)min_depth, fx, fy, d_jobs, d_ranks, n_ranks,
              d_points, capacity);
    return check_launch("cloud_expand_batch_kernel");
}

extern "C" size_t vlfm_dbscan_batch_scratch_bytes(int n) {
    if (n <= 0) return 0;
    const size_t cb = ((size_t)n + 63) / 64;
    return ((size_t)n * cb * 8 + (size_t)4 * n * sizeof(int32_t) + 255) & ~(size_t)255;
}

extern "C" int vlfm_dbscan_largest_cluster_batch(const double* d_points, int capacity, const int64_t* d_jobs, int n_jobs, int max_n,
                                                 double eps, int min_points, void* d_scratch, size_t scratch_bytes, double* d_kept,
                                                 int32_t* d_num_keep, void* stream) {
    if (n_jobs == 0) return VLFM_OK;
    if (!d_points || !d_jobs || !d_kept || !d_num_keep || capacity <= 0 || n_jobs < 0 || n_jobs > 65535 || max_n < 0 ||
        max_n > 8192 || min_points < 1 || !(eps > 0) || (max_n > 0 && !d_scratch))
        return fail(VLFM_ERR_INVALID, "dbscan_batch: bad argument (n <= 8192 per job)");
    if (scratch_bytes < vlfm_dbscan_batch_scratch_bytes(max_n)) return fail(VLFM_ERR_CAPACITY, "dbscan_batch: scratch too small");
    if (max_n > 0) {
        VLFM_TIMED("dbscan_adjacency_batch_kernel", stream);
        OC_LAUNCH(dbscan_adjacency_batch_kernel, dim3((max_n + 3) / 4, n_jobs), dim3(256), 0, stream, d_points, capacity,
                  (const long long*)d_jobs, max_n, eps * eps, d_scratch, scratch_bytes);
    }
    VLFM_TIMED("dbscan_cluster_batch_kernel", stream);
    OC_LAUNCH(dbscan_cluster_batch_kernel, dim3(n_jobs), dim3(1024), 0, stream, d_points, capacity, (const long long*)d_jobs, max_n,
              min_points, d_scratch, scratch_bytes, d_kept, d_num_keep);
    return check_launch("dbscan_cluster_batch_kernel");
}
