// tvam_report.hip — the print report's one primitive (drtvam_amd/utils.py: iou_sweep, save_histogram;
// the reference's save_histogram, utils.py:8-11, :48-81): the class-split histogram of the dose over
// a sorted edge table, one pass over dose and target, exact integer counts.
//
//   class c = target > 0 ? 1 : 0, slot j = #{k : edges[k] < x} (side 0) or #{k : edges[k] <= x}
//   (side 1), counts[c][j]; a NaN x takes no slot and is counted in counts[c][n_edges + 1].
//
// The IoU of (x > edges[k]) against the object mask for every k is two suffix sums of the side-0
// counts, and the half-open dose histogram is the side-1 counts: what the reference finds in 300
// compare / and / or / count passes over the volume.
//
// Kernel: 256 threads, grid-stride.  The edge table sits in LDS; a lane finds its slot with the
// branch-free lower bound (one LDS read, one fp32 compare and one select per step over a uniform
// length: floor(log2 n_edges) steps and a last compare, 11 + 1 at 2048 edges, whose 2049 outcomes
// need 12 compares).  The steps of one search wait on each other's LDS read, so the 8 entries of a
// thread's two float4s are searched side by side (0.25 -> 0.167 ms at 64e6 entries).  Only fp32
// compares touch x, so the slot is exact: -0 == 0, +-inf land in slot 0 or n_edges, denormals
// compare as themselves (the build keeps fp32 denormals: no flush flag, denorm mode 3 in the kernel
// descriptor).
// Counters are u32 in LDS, one copy per wave (per wave pair above 1024 edges, to stay under 64 KiB),
// flushed with one 64-bit global atomic add per non-zero slot.  A converged dose is bimodal: the
// lanes of a wave want the same few counters, at worst the same one or two.  Same-address LDS adds
// cost little until most of a wave shares one (a 0.85 +- 0.02 / 0.97 +- 0.01 dose runs as fast as a
// uniform one, two exact spikes 1.7 x slower), so the wave folds only then: when 8 or more lanes
// hold the first lane's key they drop out and one lane adds their number, once more for the next
// key, and what is left goes to LDS one add per lane (hist_count; measurements in DESIGN.md 4h).
// A workgroup consumes fewer than 2^32 entries between flushes: the host splits longer vectors into
// launches of at most 2^31 entries per workgroup.
// Main path: non-temporal float4 loads from the 16-byte grid, two in flight per vector and thread,
// scalar head and tail; x and target at different offsets from that grid take the scalar path
// whole.  No scratch, no dynamically indexed per-thread arrays.
#include "tvam_plan.h"

#include <algorithm>
#include <cmath>

#define TVAM_RB 256          // threads per workgroup
#define TVAM_R_GRID 2048     // most workgroups of a launch (1024: 0.167 ms, 2048: 0.145 ms, profiles/report/)
#define TVAM_R_MAX_EDGES 2048
#define TVAM_R_FOLD_MIN 8    // lanes that must share a key for the wave to fold it

namespace {

struct HistArgs {
    const float* x;
    const float* target;
    uint64_t n, head;  // head: leading entries of the scalar path
    const float* edges;
    int32_t n_edges;
    int32_t copy_shift;  // wave w adds into counter copy w >> copy_shift
    unsigned long long* counts;
};

__device__ __forceinline__ float4 hist_ld4(const float* p, uint64_t i) {
    typedef float vf4 __attribute__((ext_vector_type(4)));
    const vf4 v = __builtin_nontemporal_load(reinterpret_cast<const vf4*>(p) + i);
    return make_float4(v.x, v.y, v.z, v.w);
}

// slot of x: the lower bound (SIDE 0) or upper bound (SIDE 1) of x in e[0, n); a NaN compares false
// at every step (slot 0) and is moved to n + 1
template <int SIDE>
__device__ __forceinline__ uint32_t hist_slot(const float* e, uint32_t n, float x) {
    uint32_t base = 0;
    for (uint32_t len = n; len > 1;) {  // len is uniform: a scalar loop, a select per lane
        const uint32_t half = len >> 1;
        const float v = e[base + half - 1];
        base += (SIDE == 0 ? v < x : v <= x) ? half : 0u;
        len -= half;
    }
    const float v = e[base];
    base += (SIDE == 0 ? v < x : v <= x) ? 1u : 0u;
    return x != x ? n + 1 : base;
}

// the slots of the 8 entries of two float4s, searched side by side: the steps of one search depend
// on each other through an LDS read, so 8 independent chains share each step's latency (the arrays
// are indexed by unrolled constants only: registers)
template <int SIDE>
__device__ __forceinline__ void hist_slot8(const float* e, uint32_t n, const float (&x)[8], uint32_t (&j)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) j[u] = 0;
    for (uint32_t len = n; len > 1;) {
        const uint32_t half = len >> 1;
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = e[j[u] + half - 1];
#pragma unroll
        for (int u = 0; u < 8; ++u) j[u] += (SIDE == 0 ? v[u] < x[u] : v[u] <= x[u]) ? half : 0u;
        len -= half;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const float v = e[j[u]];
        j[u] += (SIDE == 0 ? v < x[u] : v <= x[u]) ? 1u : 0u;
        j[u] = x[u] != x[u] ? n + 1 : j[u];
    }
}

// One entry into this wave's counter copy.  FOLD: up to two rounds in which the lanes that hold the first remaining lane's key drop out and
// one of them adds their number; MIN: a round (and the next) only runs when at least MIN lanes share
// that key, a wave-uniform test, so a spread-out dose pays one ballot and no extra LDS add
template <int FOLD, int MIN>
__device__ __forceinline__ void hist_count(uint32_t* cnt, uint32_t key) {
    bool todo = true;
    if (FOLD) {
        const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
        const bool same = key == k0;
        const unsigned long long m = __ballot(same);  // of the lanes that are here
        if (__popcll(m) >= MIN) {
            if (same && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(&cnt[k0], (uint32_t)__popcll(m));
            todo = !same;
            if (todo) {
                const uint32_t k1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
                const bool same1 = key == k1;
                const unsigned long long m1 = __ballot(same1);
                if (__popcll(m1) >= MIN) {
                    if (same1 && (int)__lane_id() == __ffsll((long long)m1) - 1)
                        atomicAdd(&cnt[k1], (uint32_t)__popcll(m1));
                    todo = !same1;
                }
            }
        }
    }
    if (todo) atomicAdd(&cnt[key], 1u);
}

template <int SIDE, int FOLD>
__device__ __forceinline__ void hist_add(const float* e, uint32_t* cnt, uint32_t n_edges, float x, float t) {
    hist_count<(FOLD != 0), (FOLD == 1 ? TVAM_R_FOLD_MIN : 1)>(
        cnt, (t > 0.0f ? n_edges + 2 : 0u) + hist_slot<SIDE>(e, n_edges, x));
}

template <int SIDE, int FOLD>
__global__ __launch_bounds__(TVAM_RB) void tvam_class_hist_kernel(HistArgs q) {
    extern __shared__ uint32_t lds[];
    const uint32_t ne = (uint32_t)q.n_edges, row = 2 * (ne + 2);
    const uint32_t copies = (TVAM_RB / 64) >> q.copy_shift;
    float* e = reinterpret_cast<float*>(lds);
    uint32_t* all = lds + ne;
    for (uint32_t i = threadIdx.x; i < ne; i += TVAM_RB) e[i] = q.edges[i];
    for (uint32_t i = threadIdx.x; i < copies * row; i += TVAM_RB) all[i] = 0u;
    __syncthreads();
    uint32_t* cnt = all + ((threadIdx.x >> 6) >> q.copy_shift) * row;

    const uint64_t stride = (uint64_t)gridDim.x * TVAM_RB;
    const uint64_t tid = (uint64_t)blockIdx.x * TVAM_RB + threadIdx.x;
    for (uint64_t i = tid; i < q.head; i += stride)
        hist_add<SIDE, FOLD>(e, cnt, ne, __builtin_nontemporal_load(q.x + i), __builtin_nontemporal_load(q.target + i));
    const float* x4 = q.x + q.head;
    const float* t4 = q.target + q.head;
    const uint64_t n4 = (q.n - q.head) / 4;
    for (uint64_t i = tid; i < n4; i += 2 * stride) {
        const uint64_t i1 = i + stride;
        const bool two = i1 < n4;
        const float4 xa = hist_ld4(x4, i), ta = hist_ld4(t4, i);
        float4 xb = xa, tb = ta;
        if (two) {
            xb = hist_ld4(x4, i1);
            tb = hist_ld4(t4, i1);
        }
        const float xs[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
        const float ts[8] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z, tb.w};
        uint32_t j[8];
        hist_slot8<SIDE>(e, ne, xs, j);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (u < 4 || two) hist_count<(FOLD != 0), (FOLD == 1 ? TVAM_R_FOLD_MIN : 1)>(cnt, (ts[u] > 0.0f ? ne + 2 : 0u) + j[u]);
    }
    for (uint64_t i = q.head + 4 * n4 + tid; i < q.n; i += stride)
        hist_add<SIDE, FOLD>(e, cnt, ne, __builtin_nontemporal_load(q.x + i), __builtin_nontemporal_load(q.target + i));

    __syncthreads();
    for (uint32_t s = threadIdx.x; s < row; s += TVAM_RB) {
        unsigned long long v = 0;
        for (uint32_t c = 0; c < copies; ++c) v += all[c * row + s];
        if (v) atomicAdd(&q.counts[s], v);
    }
}

// Entries up to the 16-byte grid when x and target sit at the same offset from it, else all n.
uint64_t hist_head(uint64_t n, const float* x, const float* target) {
    const uintptr_t ox = (uintptr_t)x & 15u, ot = (uintptr_t)target & 15u;
    if (ox != ot) return n;
    return std::min<uint64_t>(n, ((16u - ox) & 15u) / 4);
}

}  // namespace

extern "C" int tvam_class_hist(const float* x, const float* target, uint64_t n, const float* edges, int32_t n_edges,
                               int32_t side, uint64_t* counts, void* hip_stream) {
    if (n_edges < 1 || n_edges > TVAM_R_MAX_EDGES)
        return tvam_fail(TVAM_ERR_INVALID, "tvam_class_hist: 1 <= n_edges <= " + std::to_string(TVAM_R_MAX_EDGES) +
                                               " (got " + std::to_string(n_edges) + ")");
    if (side != 0 && side != 1)
        return tvam_fail(TVAM_ERR_INVALID, "tvam_class_hist: side must be 0 or 1 (got " + std::to_string(side) + ")");
    if (!edges || !counts || (n > 0 && (!x || !target))) return tvam_fail(TVAM_ERR_INVALID, "tvam_class_hist: null argument");
    for (int32_t k = 0; k < n_edges; ++k) {
        if (!std::isfinite(edges[k]))
            return tvam_fail(TVAM_ERR_INVALID, "tvam_class_hist: edge " + std::to_string(k) + " is not finite");
        if (k > 0 && !(edges[k - 1] < edges[k]))
            return tvam_fail(TVAM_ERR_INVALID, "tvam_class_hist: edges must be strictly increasing (edge " +
                                                   std::to_string(k) + " <= edge " + std::to_string(k - 1) + ")");
    }
    if ((((uintptr_t)x | (uintptr_t)target) & 3u) != 0 || ((uintptr_t)counts & 7u) != 0)
        return tvam_fail(TVAM_ERR_INVALID, "tvam_class_hist: x and target must be 4-byte aligned, counts 8-byte aligned");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t row = 2 * ((size_t)n_edges + 2);
    hipError_t err = hipMemsetAsync(counts, 0, row * sizeof(uint64_t), stream);
    if (err != hipSuccess) return tvam_hip_fail(err, "tvam_class_hist: hipMemsetAsync");
    TvamDevBuf<float> dev_edges;  // freed on return, after the synchronisation
    if (n > 0) {
        if ((err = dev_edges.alloc((size_t)n_edges)) != hipSuccess) return tvam_hip_fail(err, "tvam_class_hist: hipMalloc");
        err = hipMemcpyAsync(dev_edges.get(), edges, (size_t)n_edges * sizeof(float), hipMemcpyHostToDevice, stream);
        if (err != hipSuccess) return tvam_hip_fail(err, "tvam_class_hist: hipMemcpyAsync");
        // the per-wave fold: 1 = when TVAM_R_FOLD_MIN lanes share a key; the A/B of DESIGN.md 4h: 0 = never, 2 = always
        const int fold = tvam_knob("TVAM_REPORT_FOLD", 1);
        // launches of at most 2^31 entries per workgroup (a multiple of 4: the parts keep x's and
        // target's offsets from the 16-byte grid), so no u32 counter wraps
        const unsigned gmax = (unsigned)std::min(std::max(tvam_knob("TVAM_REPORT_GRID", TVAM_R_GRID), 1), 8192);
        const uint64_t part_max = (uint64_t)gmax << 31;
        for (uint64_t off = 0; off < n; off += part_max) {
            HistArgs q;
            q.x = x + off;
            q.target = target + off;
            q.n = std::min(n - off, part_max);
            q.head = hist_head(q.n, q.x, q.target);
            q.edges = dev_edges.get();
            q.n_edges = n_edges;
            q.copy_shift = n_edges <= 1024 ? 0 : 1;
            q.counts = reinterpret_cast<unsigned long long*>(counts);
            const uint64_t items = q.head == q.n ? q.n : (q.n - q.head) / 4 + 8;
            const dim3 grid((unsigned)std::min<uint64_t>((items + TVAM_RB - 1) / TVAM_RB, gmax)), block(TVAM_RB);
            const size_t lds = ((size_t)n_edges + ((TVAM_RB / 64) >> q.copy_shift) * row) * sizeof(uint32_t);
            auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, lds, stream, q); };
            if (side == 0)
                fold == 0 ? go(tvam_class_hist_kernel<0, 0>) : fold == 2 ? go(tvam_class_hist_kernel<0, 2>)
                                                                         : go(tvam_class_hist_kernel<0, 1>);
            else
                fold == 0 ? go(tvam_class_hist_kernel<1, 0>) : fold == 2 ? go(tvam_class_hist_kernel<1, 2>)
                                                                         : go(tvam_class_hist_kernel<1, 1>);
            if ((err = hipGetLastError()) != hipSuccess) return tvam_hip_fail(err, "tvam_class_hist: launch");
        }
    }
    if ((err = hipStreamSynchronize(stream)) != hipSuccess) return tvam_hip_fail(err, "tvam_class_hist");
    return 0;
}
