// cloud_query.hip -- the two per-step questions ObjectPointCloudMap asks of its accumulated clouds, for MANY clouds in one launch,
// over device mirrors of the clouds (vlfm_amd/mapping/object_point_cloud_map.py: update_explored_batch, get_best_objects_batch):
//
//   cone:     which far-tag slots of a cloud have a point inside the view cone (within_fov_cone, geometry_utils.py:91-116, as
//             update_explored uses it, object_point_cloud_map.py:103-135)
//   closest:  the first index of the minimum of norm(cloud[:, :k] - position) over the trusted points and over all points, and
//             the number of trusted points (get_target_cloud + _get_closest_point, :137-144, :172-183)
//
// A cloud is [n][4] f64 rows (x, y, z, tag), 32 bytes each, read as two 16-byte loads; its slot array is [n] i32: -1 for tag 1.0
// (trusted), else the index of the tag in the cloud's host table.  The grid is (chunk of CQ_CHUNK points, query); a workgroup reads
// its query's row of the device table and leaves at once when its chunk lies behind the cloud's end.
//
// Arithmetic: every f64 operation is rounded on its own (__dmul_rn / __dadd_rn, the build passes -ffp-contract=off), in NumPy's
// order: norm(axis=1) of 2 or 3 columns is sqrt((dx*dx + dy*dy) + dz*dz).  sqrt(double) is the correctly rounded IEEE root, and the
// comparisons are made on the ROOTS as NumPy makes them (two different sums of squares can round to one root).  atan2 is the one
// function that cannot be assumed bit-equal to NumPy's libm: a far point whose |angle difference| lies within CQ_BAND of half the
// field of view is neither included nor excluded here but reported as UNCERTAIN, and the host decides it with NumPy.
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vlfm_amd.h"
#include "profile.h"
#include "status.h"

namespace vlfm {

constexpr int CQ_THREADS = 256;                    // 4 wavefronts of 64
constexpr int CQ_PER_THREAD = 16;
constexpr int CQ_CHUNK = CQ_THREADS * CQ_PER_THREAD;   // 4096 points = 128 KB of rows per workgroup
constexpr double CQ_BAND = 1e-9;
constexpr double CQ_PI = 3.141592653589793;        // np.pi

static_assert(sizeof(vlfm_cloud_query) == 80, "vlfm_cloud_query is 80 bytes (the host fills it as a NumPy record)");

__device__ inline double cq_sub(double a, double b) { return __dadd_rn(a, -b); }

// np.linalg.norm((x, y[, z]) - p) for one row
__device__ inline double cq_dist(double2 xy, double z, const double* p, int k) {
    const double dx = cq_sub(xy.x, p[0]), dy = cq_sub(xy.y, p[1]);
    double s = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
    if (k == 3) {
        const double dz = cq_sub(z, p[2]);
        s = __dadd_rn(s, __dmul_rn(dz, dz));
    }
    return sqrt(s);
}

// ---------------------------------------------------------------------------------------------- cone
// flags [.. + 0 .. n_slots) = 1: the slot has a point inside the cone; [.. + n_slots .. 2 n_slots) = 1: it has a point in the band.
// Every writer stores the same 1 (plain vector stores; the host zeroes the flags before the launch).
__global__ __launch_bounds__(CQ_THREADS) void cloud_cone_kernel(const vlfm_cloud_query* __restrict__ queries,
                                                                int32_t* __restrict__ flags) {
    const vlfm_cloud_query Q = queries[blockIdx.y];
    const int first = blockIdx.x * CQ_CHUNK;
    if (first >= Q.n) return;
    const int end = min(Q.n, first + CQ_CHUNK);
    const double2* rows = (const double2*)Q.d_rows;
    int32_t* in = flags + Q.flag_offset;
    int32_t* band = in + Q.n_slots;
    for (int i = first + threadIdx.x; i < end; i += CQ_THREADS) {
        const int slot = Q.d_slots[i];
        if (slot < 0 || slot >= Q.n_slots) continue;          // trusted points are never dropped (`- {1}`)
        const double2 xy = rows[2 * (size_t)i], zt = rows[2 * (size_t)i + 1];
        const double dx = cq_sub(xy.x, Q.p[0]), dy = cq_sub(xy.y, Q.p[1]), dz = cq_sub(zt.x, Q.p[2]);
        const double dist = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
        if (!(dist <= Q.range)) continue;
        // np.mod(angles - cone_angle + np.pi, 2 * np.pi) - np.pi: the remainder takes the sign of the divisor
        const double x = __dadd_rn(cq_sub(atan2(dy, dx), Q.heading), CQ_PI);
        double m = fmod(x, 2.0 * CQ_PI);
        if (m < 0.0) m = __dadd_rn(m, 2.0 * CQ_PI);
        const double a = fabs(cq_sub(m, CQ_PI));
        if (fabs(cq_sub(a, Q.half_fov)) < CQ_BAND)
            band[slot] = 1;
        else if (a <= Q.half_fov)
            in[slot] = 1;
    }
}

// ---------------------------------------------------------------------------------------------- closest
// (distance, index) pairs are ordered by distance, then by index: the minimum of that order is np.argmin's "first index of the
// minimum" however the pairs are grouped, so the reduction is deterministic without any atomic.
struct CqBest {
    double d;
    int i;
};
__device__ inline bool cq_less(double d, int i, const CqBest& b) { return d < b.d || (d == b.d && i < b.i); }

// partial [query][chunk] = 4 x f64 words: trusted distance, all distance, then (trusted index, all index), (trusted count, 0) as i32
constexpr int CQ_PARTIAL_WORDS = 4;

__global__ __launch_bounds__(CQ_THREADS) void cloud_closest_partial_kernel(const vlfm_cloud_query* __restrict__ queries,
                                                                           int max_chunks, double* __restrict__ partials) {
    __shared__ double s_d[2][CQ_THREADS];
    __shared__ int s_i[2][CQ_THREADS];
    __shared__ int s_n[CQ_THREADS];
    const vlfm_cloud_query Q = queries[blockIdx.y];
    const int first = blockIdx.x * CQ_CHUNK;
    if (first >= Q.n) return;
    const int end = min(Q.n, first + CQ_CHUNK);
    const double2* rows = (const double2*)Q.d_rows;
    const double inf = __longlong_as_double(0x7FF0000000000000LL);
    CqBest trusted{inf, 0x7FFFFFFF}, all{inf, 0x7FFFFFFF};
    int count = 0;
    for (int i = first + threadIdx.x; i < end; i += CQ_THREADS) {
        const double2 xy = rows[2 * (size_t)i], zt = rows[2 * (size_t)i + 1];
        const double d = cq_dist(xy, zt.x, Q.p, Q.k);
        if (cq_less(d, i, all)) all = CqBest{d, i};
        if (zt.y == 1.0) {
            count++;
            if (cq_less(d, i, trusted)) trusted = CqBest{d, i};
        }
    }
    const int t = threadIdx.x;
    s_d[0][t] = trusted.d, s_i[0][t] = trusted.i, s_d[1][t] = all.d, s_i[1][t] = all.i, s_n[t] = count;
    __syncthreads();
    for (int half = CQ_THREADS / 2; half > 0; half >>= 1) {
        if (t < half) {
            for (int w = 0; w < 2; w++) {
                const CqBest mine{s_d[w][t], s_i[w][t]};
                if (cq_less(s_d[w][t + half], s_i[w][t + half], mine)) s_d[w][t] = s_d[w][t + half], s_i[w][t] = s_i[w][t + half];
            }
            s_n[t] += s_n[t + half];
        }
        __syncthreads();
    }
    if (t == 0) {
        double* out = partials + ((size_t)blockIdx.y * max_chunks + blockIdx.x) * CQ_PARTIAL_WORDS;
        int* oi = (int*)(out + 2);
        out[0] = s_d[0][0], out[1] = s_d[1][0];
        oi[0] = s_i[0][0], oi[1] = s_i[1][0], oi[2] = s_n[0], oi[3] = 0;
    }
}

// one wavefront per query: the chunks' partials to (trusted points, first trusted minimum or -1, first minimum or -1, 0)
__global__ __launch_bounds__(64) void cloud_closest_final_kernel(const vlfm_cloud_query* __restrict__ queries, int max_chunks,
                                                                 const double* __restrict__ partials, int32_t* __restrict__ result) {
    __shared__ double s_d[2][64];
    __shared__ int s_i[2][64];
    __shared__ int s_n[64];
    const int n = queries[blockIdx.x].n;
    const int chunks = (n + CQ_CHUNK - 1) / CQ_CHUNK;
    const double inf = __longlong_as_double(0x7FF0000000000000LL);
    CqBest trusted{inf, 0x7FFFFFFF}, all{inf, 0x7FFFFFFF};
    int count = 0;
    const int t = threadIdx.x;
    for (int c = t; c < chunks && c < max_chunks; c += 64) {
        const double* in = partials + ((size_t)blockIdx.x * max_chunks + c) * CQ_PARTIAL_WORDS;
        const int* ii = (const int*)(in + 2);
        if (cq_less(in[0], ii[0], trusted)) trusted = CqBest{in[0], ii[0]};
        if (cq_less(in[1], ii[1], all)) all = CqBest{in[1], ii[1]};
        count += ii[2];
    }
    s_d[0][t] = trusted.d, s_i[0][t] = trusted.i, s_d[1][t] = all.d, s_i[1][t] = all.i, s_n[t] = count;
    __syncthreads();
    for (int half = 32; half > 0; half >>= 1) {
        if (t < half) {
            for (int w = 0; w < 2; w++) {
                const CqBest mine{s_d[w][t], s_i[w][t]};
                if (cq_less(s_d[w][t + half], s_i[w][t + half], mine)) s_d[w][t] = s_d[w][t + half], s_i[w][t] = s_i[w][t + half];
            }
            s_n[t] += s_n[t + half];
        }
        __syncthreads();
    }
    if (t == 0) {
        int32_t* out = result + 4 * (size_t)blockIdx.x;
        out[0] = s_n[0];
        out[1] = s_i[0][0] == 0x7FFFFFFF ? -1 : s_i[0][0];
        out[2] = s_i[1][0] == 0x7FFFFFFF ? -1 : s_i[1][0];
        out[3] = 0;
    }
}

}  // namespace vlfm

using namespace vlfm;

static std::atomic<long long> g_launches{0};
#define CQ_LAUNCH(...)             \
    do {                           \
        g_launches.fetch_add(1);   \
        VLFM_KLAUNCH(__VA_ARGS__); \
    } while (0)

extern "C" long long vlfm_cloud_query_launch_count(void) { return g_launches.load(); }

extern "C" int vlfm_cloud_query_chunk(void) { return CQ_CHUNK; }

static int cq_chunks(int n_queries, int max_points, const char** why) {
    if (n_queries < 0 || n_queries > 65535 || max_points < 0) {
        *why = "cloud_query: bad argument (queries <= 65535)";
        return -1;
    }
    return (max_points + CQ_CHUNK - 1) / CQ_CHUNK;
}

extern "C" int vlfm_cloud_cone_flags(const vlfm_cloud_query* d_queries, int n_queries, int max_points, int32_t* d_flags,
                                     void* stream) {
    const char* why = nullptr;
    const int chunks = cq_chunks(n_queries, max_points, &why);
    if (chunks < 0) return fail(VLFM_ERR_INVALID, why);
    if (n_queries == 0 || chunks == 0) return VLFM_OK;
    if (!d_queries || !d_flags) return fail(VLFM_ERR_INVALID, "cloud_cone_flags: null pointer");
    VLFM_TIMED("cloud_cone_kernel", stream);
    CQ_LAUNCH(cloud_cone_kernel, dim3(chunks, n_queries), dim3(CQ_THREADS), 0, stream, d_queries, d_flags);
    return check_launch("cloud_cone_kernel");
}

extern "C" size_t vlfm_cloud_closest_scratch_bytes(int n_queries, int max_points) {
    if (n_queries <= 0 || max_points <= 0) return 0;
    return (size_t)n_queries * ((max_points + CQ_CHUNK - 1) / CQ_CHUNK) * CQ_PARTIAL_WORDS * sizeof(double);
}

extern "C" int vlfm_cloud_closest(const vlfm_cloud_query* d_queries, int n_queries, int max_points, void* d_scratch,
                                  size_t scratch_bytes, int32_t* d_result, void* stream) {
    const char* why = nullptr;
    const int chunks = cq_chunks(n_queries, max_points, &why);
    if (chunks < 0) return fail(VLFM_ERR_INVALID, why);
    if (n_queries == 0) return VLFM_OK;
    if (!d_queries || !d_result || (chunks > 0 && !d_scratch)) return fail(VLFM_ERR_INVALID, "cloud_closest: null pointer");
    if (scratch_bytes < vlfm_cloud_closest_scratch_bytes(n_queries, max_points))
        return fail(VLFM_ERR_CAPACITY, "cloud_closest: scratch too small");
    if (chunks > 0) {
        VLFM_TIMED("cloud_closest_partial_kernel", stream);
        CQ_LAUNCH(cloud_closest_partial_kernel, dim3(chunks, n_queries), dim3(CQ_THREADS), 0, stream, d_queries, chunks,
                  (double*)d_scratch);
    }
    VLFM_TIMED("cloud_closest_final_kernel", stream);
    CQ_LAUNCH(cloud_closest_final_kernel, dim3(n_queries), dim3(64), 0, stream, d_queries, chunks, (const double*)d_scratch,
              d_result);
    return check_launch("cloud_closest_final_kernel");
}
