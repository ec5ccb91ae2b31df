// k_gdn.hip — the guided denoiser of include/rpt.h ("guided denoiser": project-defined): the a-trous filter of denoise.hip with the
// normal and position buffers of Dammertz et al. restored, a key that no tap crosses, and albedo demodulation.  A code object library of
// its own (build.py, gdn_lib_of; launch_gdn.h): no other library gains or loses a kernel.  The specification is the header's text; the
// float32 restatement the kernels are held to, bit for bit, is tests/gdn_np.py.
//
// Roofline: HBM.  A pixel is 16 B of colour and 64 B of rpt_guide, of which a TAP reads 48 B: the compressed colour and the guide's first
// two 16-byte lines (position + key, ns + t); the third (ng) and fourth (albedo) lines are the centre's alone.  The first iterations
// (steps 1 and 2) are FUSED through LDS as in denoise.hip: a 32 x 16 tile plus a halo of 1 + 2 pixels — 38 x 22 cells of 32 B of guide and
// 12 B of compressed colour, and 36 x 20 cells of colour for the second stage: 45.5 KB, three workgroups of 512 lanes per CU.  (The
// colour-only filter fuses three iterations on 32 x 32 tiles at 12 B per cell; at 44 B per cell that shape needs 110 KB.)  Later
// iterations read their taps through L1 / L2 (gdn_step_kernel).  -DRPT_GDN_UNFUSED: one pass per iteration (A/B; profiles/NOTES.md).
// Halo pixels of the first stage are computed by every tile that needs them: the same operations on the same values, so the bits do
// not depend on the form.  Built like denoise.hip: -fslp-vectorize, -DRPT_GUARD_PER_OP (every divide is the IEEE quotient).
#include <hip/hip_runtime.h>

#include "dev_math.h"
#include "launch_gdn.h"

using namespace rptdev;

namespace {

constexpr float kGdnFloor = 1.0f / 64.0f;                             // the albedo floor of demodulation (rpt.h: FLOOR)

struct GdnSum {
    v3 acc;
    float wsum;
};

// What a pixel keeps of itself while its nine taps are weighed.
struct GdnCentre {
    v3 c;                                                            // compressed colour
    v3 pos, ns, ng;
    uint32_t key;
    float kx;                                                        // plane_k / t^2, or 0
};

struct GdnCell { float x, y, z; };                                   // a compressed colour in LDS

RPT_DEV float gdn_h(int d) { return d == 0 ? 0.5f : 0.25f; }
RPT_DEV float gdn_sq3(float a, float b, float c) { return __builtin_fmaf(a, a, __builtin_fmaf(b, b, c * c)); }
RPT_DEV float gdn_floor(float a) { return a < kGdnFloor ? kGdnFloor : a; }     // (a NaN albedo stays a NaN)
RPT_DEV float gdn_kx(float plane_k, float t) { return plane_k > 0.0f ? fdiv(plane_k, t * t) : 0.0f; }

// c' = e / (1 + e), e = c / max(albedo, FLOOR)
RPT_DEV GdnCell gdn_compress(float4 c, float4 alb)
{
    const float e0 = fdiv(c.x, gdn_floor(alb.x)), e1 = fdiv(c.y, gdn_floor(alb.y)), e2 = fdiv(c.z, gdn_floor(alb.z));
    return GdnCell{fdiv(e0, 1.0f + e0), fdiv(e1, 1.0f + e1), fdiv(e2, 1.0f + e2)};
}

// one tap (rpt.h: the key test, d2 / dn2 / dp2 and their skip, the three edge-stopping factors).  g0 = position + key, g1 = ns + t.
RPT_DEV void gdn_tap(GdnSum& s, const GdnCentre& p, v3 cq, float4 g0, float4 g1, float hw, float k, float normal_k)
{
    if (__float_as_uint(g0.w) != p.key) return;
    const float inf = __builtin_inff();
    const float d2 = gdn_sq3(p.c.x - cq.x, p.c.y - cq.y, p.c.z - cq.z);
    const float dn2 = gdn_sq3(p.ns.x - g1.x, p.ns.y - g1.y, p.ns.z - g1.z);
    const float r0 = g0.x - p.pos.x, r1 = g0.y - p.pos.y, r2 = g0.z - p.pos.z;
    const float dpl = __builtin_fmaf(p.ng.x, r0, __builtin_fmaf(p.ng.y, r1, p.ng.z * r2));
    const float dp2 = dpl * dpl;
    if (!(d2 < inf) || !(dn2 < inf) || !(dp2 < inf)) return;
    const float tc = __builtin_fmaf(-d2, k, 1.0f), tn = __builtin_fmaf(-dn2, normal_k, 1.0f), tx = __builtin_fmaf(-dp2, p.kx, 1.0f);
    const float gc = tc > 0.0f ? tc : 0.0f, gn = tn > 0.0f ? tn : 0.0f, gx = tx > 0.0f ? tx : 0.0f;
    const float wt = ((hw * (gc * gc)) * (gn * gn)) * (gx * gx);
    s.acc.x = __builtin_fmaf(cq.x, wt, s.acc.x);
    s.acc.y = __builtin_fmaf(cq.y, wt, s.acc.y);
    s.acc.z = __builtin_fmaf(cq.z, wt, s.acc.z);
    s.wsum = s.wsum + wt;
}

// The pixel's new compressed colour; in the last iteration the expanded, remodulated pixel (or the input, copied through).
RPT_DEV float4 gdn_finish(const GdnSum& s, v3 cp, bool last, float4 orig, float4 alb)
{
    const bool ok = s.wsum > 0.0f;
    const v3 m = divs3(s.acc, s.wsum);
    const v3 o = mk3(ok ? m.x : cp.x, ok ? m.y : cp.y, ok ? m.z : cp.z);
    if (!last) return make_float4(o.x, o.y, o.z, 0.0f);
    const float inf = __builtin_inff();
    const float a0 = gdn_floor(alb.x), a1 = gdn_floor(alb.y), a2 = gdn_floor(alb.z);
    const float e0 = fdiv(orig.x, a0), e1 = fdiv(orig.y, a1), e2 = fdiv(orig.z, a2);      // stage 0's e, recomputed: the same bits
    const bool finite = (__builtin_fabsf(e0) < inf) && (__builtin_fabsf(e1) < inf) && (__builtin_fabsf(e2) < inf) &&
                        e0 != -1.0f && e1 != -1.0f && e2 != -1.0f;
    if (!finite) return orig;
    return make_float4(fdiv(o.x, 1.0f - o.x) * a0, fdiv(o.y, 1.0f - o.y) * a1, fdiv(o.z, 1.0f - o.z) * a2, orig.w);
}

// rpt_guide as four 16-byte lines
constexpr uint32_t kLinePos = 0u, kLineNs = 1u, kLineNg = 2u, kLineAlbedo = 3u;
RPT_DEV float4 gdn_line(const float4* __restrict__ guides, size_t p, uint32_t line) { return guides[4u * p + line]; }

// ---- rpt_denoise_guides_device ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gdn_pack_kernel(const float4* __restrict__ rays, const float4* __restrict__ hits, const float4* __restrict__ surfaces,
                                                       uint64_t n, float4* __restrict__ guides)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 h0 = hits[2u * i];                                  // t, kind, primitive, mesh
    const uint32_t kind = __float_as_uint(h0.y);
    float4 l0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), l1 = make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
    float4 l2 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kind)), l3 = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    if (kind != (uint32_t)RPT_HIT_NONE) {
        const float4 r0 = rays[2u * i], r1 = rays[2u * i + 1u];      // origin, max_dist; direction, reserved
        const float4 s0 = surfaces[4u * i], s1 = surfaces[4u * i + 1u], s2 = surfaces[4u * i + 2u];   // ng.xyz ns.x; ns.yz rgb.xy; rgb.z ...
        const float t = h0.x;
        const uint32_t id = kind == (uint32_t)RPT_HIT_TRIANGLE ? __float_as_uint(h0.w) : __float_as_uint(h0.z);
        const uint32_t key = (kind << 28) | (id & 0x0FFFFFFFu);
        l0 = make_float4(r0.x + r1.x * t, r0.y + r1.y * t, r0.z + r1.z * t, __uint_as_float(key));
        l1 = make_float4(s0.w, s1.x, s1.y, t);
        l2 = make_float4(s0.x, s0.y, s0.z, __uint_as_float(kind));
        l3 = make_float4(s1.z, s1.w, s2.x, 0.0f);
    }
    guides[4u * i] = l0; guides[4u * i + 1u] = l1; guides[4u * i + 2u] = l2; guides[4u * i + 3u] = l3;
}

// ---- the first K iterations (K = 1, 2; steps 1, 2) in one kernel ------------------------------------------------------------------------
// Stage 0 is the loaded region (colours compressed once per loaded pixel, the taps' 32 B of guide beside them), stage j the output of
// iteration j - 1 on the region later iterations still need; positions outside the image hold NaN colours at every stage — a tap there
// is skipped, exactly as a tap outside the image is in gdn_step_kernel.  Guides are never filtered: every stage reads stage 0's.
constexpr int kGdnTileW = 32, kGdnTileH = 16;
constexpr uint32_t kGdnThreads = (uint32_t)(kGdnTileW * kGdnTileH);
template <int K> struct GdnGeom {
    static constexpr int kHalo = (1 << K) - 1;                       // 1, 3
    static constexpr int halo(int stage) { return kHalo - ((1 << stage) - 1); }
    static constexpr int w(int stage) { return kGdnTileW + 2 * halo(stage); }
    static constexpr int h(int stage) { return kGdnTileH + 2 * halo(stage); }
    static constexpr int cells(int stage) { return K > stage ? w(stage) * h(stage) : 0; }
};

template <int K>
__global__ __launch_bounds__(kGdnThreads) void gdn_fused_kernel(const float4* __restrict__ src, const float4* __restrict__ guides, float4* __restrict__ out,
                                                                uint32_t w, uint32_t h, float k0, float normal_k, float plane_k, uint32_t last)
{
    typedef GdnGeom<K> G;
    static_assert(K == 1 || K == 2, "two colour buffers: stage 0 and stage 1");
    __shared__ float4 s_g0[G::cells(0)];                             // position + key        K = 2: 836 cells x (16 + 16 + 12) B + 720 x 12 B = 45.4 KB
    __shared__ float4 s_g1[G::cells(0)];                             // ns + t
    __shared__ GdnCell s_a[G::cells(0)];
    __shared__ GdnCell s_b[G::cells(1) > 0 ? G::cells(1) : 1];
    const int x0 = (int)blockIdx.x * kGdnTileW, y0 = (int)blockIdx.y * kGdnTileH;
    const float nan = __builtin_nanf("");
    {   // stage 0: load + compress
        constexpr int W0 = G::w(0), H0 = G::h(0), R = G::kHalo;
        for (uint32_t e = threadIdx.x; e < (uint32_t)(W0 * H0); e += kGdnThreads) {
            const int lx = (int)(e % (uint32_t)W0), ly = (int)(e / (uint32_t)W0);
            const int gx = x0 + lx - R, gy = y0 + ly - R;
            GdnCell c{nan, nan, nan};                                // outside the image: NaN, i.e. a tap that is skipped
            float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0;
            if (gx >= 0 && gy >= 0 && gx < (int)w && gy < (int)h) {
                const size_t p = (size_t)gy * w + (size_t)gx;
                g0 = gdn_line(guides, p, kLinePos);
                g1 = gdn_line(guides, p, kLineNs);
                c = gdn_compress(src[p], gdn_line(guides, p, kLineAlbedo));
            }
            s_g0[e] = g0; s_g1[e] = g1; s_a[e] = c;
        }
    }
    __syncthreads();
    float k = k0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const GdnCell* from = (j & 1) ? s_b : s_a;
        GdnCell* to = (j & 1) ? s_a : s_b;
        const int Ws = G::w(j), Wd = G::w(j + 1), Hd = G::h(j + 1), step = 1 << j;   // source stage j -> destination stage j + 1 (the tile itself when j + 1 == K)
        const int Rd = G::halo(j + 1);                                               // halo of the destination region
        const int W0 = G::w(0), off0 = G::kHalo - Rd;                                // the destination's cells within stage 0 (the guides')
        const bool to_global = j + 1 == K;
        for (uint32_t e = threadIdx.x; e < (uint32_t)(Wd * Hd); e += kGdnThreads) {
            const int lx = (int)(e % (uint32_t)Wd), ly = (int)(e / (uint32_t)Wd);
            const int gx = x0 + lx - Rd, gy = y0 + ly - Rd;
            const bool inside = gx >= 0 && gy >= 0 && gx < (int)w && gy < (int)h;
            const int ce = (ly + step) * Ws + lx + step;                             // the centre within stage j
            const int ge = (ly + off0) * W0 + lx + off0;                             // ... and within stage 0
            GdnCell o{nan, nan, nan};
            float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (inside) {
                const size_t p = (size_t)gy * w + (size_t)gx;
                const GdnCell cc = from[ce];
                const float4 c0 = s_g0[ge], c1 = s_g1[ge], c2 = gdn_line(guides, p, kLineNg);
                GdnCentre ctr;
                ctr.c = mk3(cc.x, cc.y, cc.z);
                ctr.pos = mk3(c0.x, c0.y, c0.z); ctr.key = __float_as_uint(c0.w);
                ctr.ns = mk3(c1.x, c1.y, c1.z);
                ctr.ng = mk3(c2.x, c2.y, c2.z);
                ctr.kx = gdn_kx(plane_k, c1.w);
                GdnSum s{mk3(0.0f, 0.0f, 0.0f), 0.0f};
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const GdnCell q = from[ce + dy * step * Ws + dx * step];
                        const int gq = ge + dy * step * W0 + dx * step;
                        gdn_tap(s, ctr, mk3(q.x, q.y, q.z), s_g0[gq], s_g1[gq], gdn_h(dy) * gdn_h(dx), k, normal_k);
                    }
                const bool fin = to_global && last != 0u;
                float4 orig = make_float4(0.0f, 0.0f, 0.0f, 0.0f), alb = orig;
                if (fin) { orig = src[p]; alb = gdn_line(guides, p, kLineAlbedo); }
                res = gdn_finish(s, ctr.c, fin, orig, alb);
                o = GdnCell{res.x, res.y, res.z};
            }
            if (to_global) {
                if (inside) out[(size_t)gy * w + (size_t)gx] = res;
            } else {
                to[e] = o;
            }
        }
        k = k * 4.0f;
        if (!to_global) __syncthreads();
    }
}

// ---- later iterations (step 2^i): taps straight from the compressed buffer and the guides -------------------------------------------------
__global__ __launch_bounds__(256) void gdn_step_kernel(const float4* __restrict__ cur, const float4* __restrict__ orig_in, const float4* __restrict__ guides,
                                                       float4* __restrict__ out, uint32_t w, uint32_t h, int step, float k, float normal_k, float plane_k,
                                                       uint32_t last)
{
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint32_t x = blockIdx.x * 16u + tx, y = blockIdx.y * 16u + ty;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const float4 c4 = cur[p];
    const float4 c0 = gdn_line(guides, p, kLinePos), c1 = gdn_line(guides, p, kLineNs), c2 = gdn_line(guides, p, kLineNg);
    GdnCentre ctr;
    ctr.c = mk3(c4.x, c4.y, c4.z);
    ctr.pos = mk3(c0.x, c0.y, c0.z); ctr.key = __float_as_uint(c0.w);
    ctr.ns = mk3(c1.x, c1.y, c1.z);
    ctr.ng = mk3(c2.x, c2.y, c2.z);
    ctr.kx = gdn_kx(plane_k, c1.w);
    GdnSum s{mk3(0.0f, 0.0f, 0.0f), 0.0f};
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const long long qx = (long long)x + (long long)step * dx, qy = (long long)y + (long long)step * dy;
            if (qx < 0 || qy < 0 || qx >= (long long)w || qy >= (long long)h) continue;
            const size_t q = (size_t)qy * w + (size_t)qx;
            const bool centre = dx == 0 && dy == 0;
            const float4 cq = centre ? c4 : cur[q];
            const float4 g0 = centre ? c0 : gdn_line(guides, q, kLinePos), g1 = centre ? c1 : gdn_line(guides, q, kLineNs);
            gdn_tap(s, ctr, mk3(cq.x, cq.y, cq.z), g0, g1, gdn_h(dy) * gdn_h(dx), k, normal_k);
        }
    float4 orig = make_float4(0.0f, 0.0f, 0.0f, 0.0f), alb = orig;
    if (last) { orig = orig_in[p]; alb = gdn_line(guides, p, kLineAlbedo); }
    out[p] = gdn_finish(s, ctr.c, last != 0u, orig, alb);
}

#ifdef RPT_GDN_UNFUSED
constexpr uint32_t kGdnFuse = 1u;                                     // one pass per iteration: the first through LDS alone (it compresses), the rest by steps
#else
constexpr uint32_t kGdnFuse = 2u;
#endif

}  // namespace

namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t gdn_pack(const rpt_ray* rays, const rpt_hit* hits, const rpt_surface* surfaces, uint64_t n, rpt_guide* guides,
                                                           hipStream_t st)
{
    (void)hipGetLastError();
    const uint64_t blocks = (n + 255u) / 256u;
    if (n == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gdn_pack_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, (const float4*)rays, (const float4*)hits, (const float4*)surfaces, n,
                       (float4*)guides);
    return hipGetLastError();
}

// `iterations` passes: in -> t0 -> t1 -> ... -> out, alternating between `out` and `scratch` so that the last one lands in `out`.
__attribute__((visibility("default"))) hipError_t gdn_filter(const float* in, const rpt_guide* guides, float* out, float* scratch, uint32_t width, uint32_t height,
                                                             uint32_t iterations, float edge_k, float normal_k, float plane_k, hipStream_t st)
{
    (void)hipGetLastError();
    const float4* g = (const float4*)guides;
    const float4* orig = (const float4*)in;
    const uint32_t nf = iterations < kGdnFuse ? iterations : kGdnFuse;
    float k = edge_k;
    const float4* cur = nullptr;
    {   // iterations 0 .. nf-1 in one kernel
        const uint32_t l = nf == iterations ? 1u : 0u;
        float4* dst = (float4*)(((iterations - nf) & 1u) ? scratch : out);
        const dim3 fgrid((width + (uint32_t)kGdnTileW - 1u) / (uint32_t)kGdnTileW, (height + (uint32_t)kGdnTileH - 1u) / (uint32_t)kGdnTileH), fwg(kGdnThreads);
#ifndef RPT_GDN_UNFUSED
        if (nf == 2u) hipLaunchKernelGGL((gdn_fused_kernel<2>), fgrid, fwg, 0, st, orig, g, dst, width, height, k, normal_k, plane_k, l);
        else
#endif
            hipLaunchKernelGGL((gdn_fused_kernel<1>), fgrid, fwg, 0, st, orig, g, dst, width, height, k, normal_k, plane_k, l);
        cur = dst;
        for (uint32_t i = 0; i < nf; ++i) k = k * 4.0f;
    }
    const dim3 grid((width + 15u) / 16u, (height + 15u) / 16u), wg(256);
    for (uint32_t i = nf; i < iterations; ++i) {
        const uint32_t l = i + 1u == iterations ? 1u : 0u;
        float4* dst = (float4*)(((iterations - 1u - i) & 1u) ? scratch : out);
        hipLaunchKernelGGL(gdn_step_kernel, grid, wg, 0, st, cur, orig, g, dst, width, height, 1 << i, k, normal_k, plane_k, l);
        cur = dst;
        k = k * 4.0f;
    }
    return hipGetLastError();
}

}  // namespace rptlaunch
