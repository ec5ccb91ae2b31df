// k_tacc.hip — temporal accumulation of include/rpt.h ("temporal accumulation": project-defined): each pixel's first hit is reprojected
// into the previous frame, the previous frame's accumulated colour, sample count and luminance moments are fetched where the previous
// guides say the same surface was seen, and the new frame is blended in.  A code object library of its own (build.py, tacc_lib_of;
// launch_tacc.h): no other library gains or loses a kernel.  The specification is the header's text; the float32 restatement the
// kernels are held to, bit for bit, is tests/tacc_np.py.
//
// Roofline: HBM.  A pixel reads 16 B of colour and 48 B of its guide (position + key, ns + t, ng + kind; the albedo line is never
// read), optionally 16 B of previous position, and writes 16 B of colour and 32 B of history; a TAP reads 32 B of the previous guide
// (position + key, ns + t) and the 32-byte previous history record — one tap in IDENTITY mode, four bilinear ones when reprojecting.
// One pixel per lane; a workgroup of 256 lanes covers a 32 x 8 tile, so a wave is two rows of 32 pixels: under a small camera motion
// its 4 x 64 taps fall on three rows of the previous frame and share their cache lines (a 64 x 1 strip would touch the same lines per
// row but shares nothing between the two rows of a tap; 8 x 8 blocks cut every 128-byte line of history into quarters).
// Three forms of one template — first frame, IDENTITY, reprojecting — picked on the host: the first two carry none of the projection.
// Built like denoise.hip: -fslp-vectorize, -DRPT_GUARD_PER_OP (every divide is the IEEE quotient), -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "dev_math.h"
#include "launch_tacc.h"

using namespace rptdev;

namespace {

constexpr uint32_t kTaccTileW = 32u, kTaccTileH = 8u;
constexpr uint32_t kTaccThreads = kTaccTileW * kTaccTileH;

RPT_DEV float tacc_dot(v3 a, v3 b) { return __builtin_fmaf(a.x, b.x, __builtin_fmaf(a.y, b.y, a.z * b.z)); }
RPT_DEV bool tacc_finite(float a) { return __builtin_fabsf(a) < __builtin_inff(); }

// What a pixel keeps of itself while its taps are tested.
struct TaccCentre {
    v3 src, ns, ng;
    uint32_t key;
    bool surface;                                                    // kind != RPT_HIT_NONE: the normal and the plane test apply
    float kx;                                                        // plane_k / dot(d, d), or 0
    float normal_min;
};

struct TaccSum {
    float r, g, b, n, m1, m2;
    float wsum;
};

// one tap (rpt.h, steps 4 and 5): q inside the image.  Reads 32 B of the previous guide and the 32-byte history record.
RPT_DEV void tacc_tap(TaccSum& s, const TaccCentre& p, const float4* __restrict__ prev_guides, const float4* __restrict__ prev_history, size_t q, float wt)
{
    const float4 h0 = prev_history[2u * q], h1 = prev_history[2u * q + 1u];      // rgb n; m1 m2 - -
    const float4 g0 = prev_guides[4u * q], g1 = prev_guides[4u * q + 1u];         // position key; ns t
    bool ok = h0.w >= 1.0f && tacc_finite(h0.x) && tacc_finite(h0.y) && tacc_finite(h0.z) && tacc_finite(h1.x) && tacc_finite(h1.y);
    ok = ok && __float_as_uint(g0.w) == p.key;
    if (p.surface) {
        const float dpl = tacc_dot(p.ng, mk3(g0.x - p.src.x, g0.y - p.src.y, g0.z - p.src.z));
        ok = ok && tacc_dot(p.ns, mk3(g1.x, g1.y, g1.z)) >= p.normal_min && __builtin_fmaf(-(dpl * dpl), p.kx, 1.0f) > 0.0f;
    }
    if (!ok) return;
    s.wsum = s.wsum + wt;
    s.r = __builtin_fmaf(h0.x, wt, s.r);
    s.g = __builtin_fmaf(h0.y, wt, s.g);
    s.b = __builtin_fmaf(h0.z, wt, s.b);
    s.n = __builtin_fmaf(h0.w, wt, s.n);
    s.m1 = __builtin_fmaf(h1.x, wt, s.m1);
    s.m2 = __builtin_fmaf(h1.y, wt, s.m2);
}

template <uint32_t FORM>
__global__ __launch_bounds__(kTaccThreads) void tacc_kernel(const TaccArgs a, const float4* __restrict__ pixels, const float4* __restrict__ guides,
                                                            const float4* __restrict__ prev_guides, const float4* __restrict__ prev_history,
                                                            const float4* __restrict__ prev_positions, float4* __restrict__ out, float4* __restrict__ history)
{
    const uint32_t x = blockIdx.x * kTaccTileW + (threadIdx.x & (kTaccTileW - 1u)), y = blockIdx.y * kTaccTileH + threadIdx.x / kTaccTileW;
    if (x >= a.width || y >= a.height) return;
    const size_t i = (size_t)y * a.width + x;
    const float4 c4 = pixels[i];
    TaccSum s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (FORM != kTaccFirst) {
        const float4 g0 = guides[4u * i], g1 = guides[4u * i + 1u], g2 = guides[4u * i + 2u];   // position key; ns t; ng kind
        TaccCentre p;
        p.key = __float_as_uint(g0.w);
        p.surface = __float_as_uint(g2.w) != (uint32_t)RPT_HIT_NONE;
        p.src = mk3(g0.x, g0.y, g0.z);
        p.ns = mk3(g1.x, g1.y, g1.z);
        p.ng = mk3(g2.x, g2.y, g2.z);
        p.normal_min = a.normal_min;
        p.kx = 0.0f;
        if (FORM == kTaccReproject && prev_positions != nullptr && p.surface) {
            const float4 pp = prev_positions[i];
            p.src = mk3(pp.x, pp.y, pp.z);
        }
        v3 d = mk3(0.0f, 0.0f, 0.0f);
        if (p.surface) {                                             // step 1
            d = mk3(p.src.x - a.o[0], p.src.y - a.o[1], p.src.z - a.o[2]);
            p.kx = a.plane_k > 0.0f ? fdiv(a.plane_k, tacc_dot(d, d)) : 0.0f;
        } else if (FORM == kTaccReproject) {
            const float W = (float)a.width, H = (float)a.height;
            const float px = fdiv((float)x, W), py = 1.0f - fdiv((float)(y + 1u), H);
            const float sh = a.cam.psx * 0.5f + px, sv = a.cam.psy * 0.5f + py;
            d = mk3((a.cam.rdx + a.cam.hx * sh) + a.cam.vx * sv, (a.cam.rdy + a.cam.hy * sh) + a.cam.vy * sv, (a.cam.rdz + a.cam.hz * sh) + a.cam.vz * sv);
        }
        if (FORM == kTaccIdentity) {
            tacc_tap(s, p, prev_guides, prev_history, i, 1.0f);
        } else {                                                     // steps 2 and 3
            const float W = (float)a.width, H = (float)a.height;
            const float lam = -tacc_dot(mk3(a.w[0], a.w[1], a.w[2]), d);
            const float pa = fdiv(tacc_dot(mk3(a.u[0], a.u[1], a.u[2]), d), lam), pb = fdiv(tacc_dot(mk3(a.v[0], a.v[1], a.v[2]), d), lam);
            const float sx = __builtin_fmaf(pa, a.gx, 0.5f), sy = __builtin_fmaf(pb, a.gy, 0.5f);
            const float fx = __builtin_fmaf(sx, W, -0.5f), fy = __builtin_fmaf(1.0f - sy, H, -0.5f);
            if (lam > 0.0f && fx > -1.0f && fx < W && fy > -1.0f && fy < H) {
                const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
                const float wx = fx - x0f, wy = fy - y0f;
                const int x0 = (int)x0f, y0 = (int)y0f;              // -1 .. width - 1, -1 .. height - 1
                const float wts[4] = {(1.0f - wx) * (1.0f - wy), wx * (1.0f - wy), (1.0f - wx) * wy, wx * wy};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int qx = x0 + (t & 1), qy = y0 + (t >> 1);
                    if (qx < 0 || qy < 0 || qx >= (int)a.width || qy >= (int)a.height) continue;
                    tacc_tap(s, p, prev_guides, prev_history, (size_t)qy * a.width + (size_t)qx, wts[t]);
                }
            }
        }
    }
    // step 6
    const uint32_t exp_mask = 0x7f800000u;
    v3 c = mk3(c4.x, c4.y, c4.z);
    if ((__float_as_uint(c.x) & exp_mask) == exp_mask || (__float_as_uint(c.y) & exp_mask) == exp_mask || (__float_as_uint(c.z) & exp_mask) == exp_mask)
        c = mk3(0.0f, 0.0f, 0.0f);
    const float L = __builtin_fmaf(0.2126f, c.x, __builtin_fmaf(0.7152f, c.y, 0.0722f * c.z));
    const float L2 = L * L;
    float4 o = make_float4(c.x, c.y, c.z, c4.w);
    float n1 = 1.0f, m1 = L, m2 = L2;
    if (FORM != kTaccFirst && s.wsum > 0.0f) {
        const float hr = fdiv(s.r, s.wsum), hg = fdiv(s.g, s.wsum), hb = fdiv(s.b, s.wsum);
        const float hn = fdiv(s.n, s.wsum), hm1 = fdiv(s.m1, s.wsum), hm2 = fdiv(s.m2, s.wsum);
        const float np1 = hn + 1.0f;
        n1 = np1 < a.n_max ? np1 : a.n_max;
        const float al = fdiv(1.0f, n1), keep = 1.0f - al;
        o.x = keep * hr + c.x * al;
        o.y = keep * hg + c.y * al;
        o.z = keep * hb + c.z * al;
        m1 = keep * hm1 + L * al;
        m2 = keep * hm2 + L2 * al;
    }
    out[i] = o;
    history[2u * i] = make_float4(o.x, o.y, o.z, n1);
    history[2u * i + 1u] = make_float4(m1, m2, 0.0f, 0.0f);
}

}  // namespace

namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t tacc_accumulate(rptscene::TaccForm form, const rptscene::TaccArgs& args, const float* pixels, const rpt_guide* guides,
                                                                  const rpt_guide* prev_guides, const rpt_history* prev_history, const float* prev_positions, float* out,
                                                                  rpt_history* history, hipStream_t st)
{
    (void)hipGetLastError();
    if (args.width == 0u || args.height == 0u || args.width > 65535u || args.height > 65535u) return hipErrorInvalidValue;
    if (form != rptscene::kTaccFirst && (!prev_guides || !prev_history)) return hipErrorInvalidValue;
    if (form == rptscene::kTaccIdentity && prev_positions) return hipErrorInvalidValue;
    const dim3 grid((args.width + kTaccTileW - 1u) / kTaccTileW, (args.height + kTaccTileH - 1u) / kTaccTileH), wg(kTaccThreads);
    const float4 *px = (const float4*)pixels, *g = (const float4*)guides, *pg = (const float4*)prev_guides, *ph = (const float4*)prev_history,
                 *pp = (const float4*)prev_positions;
    float4 *o = (float4*)out, *h = (float4*)history;
    switch (form) {
    case rptscene::kTaccFirst: hipLaunchKernelGGL((tacc_kernel<rptscene::kTaccFirst>), grid, wg, 0, st, args, px, g, pg, ph, pp, o, h); break;
    case rptscene::kTaccIdentity: hipLaunchKernelGGL((tacc_kernel<rptscene::kTaccIdentity>), grid, wg, 0, st, args, px, g, pg, ph, pp, o, h); break;
    default: hipLaunchKernelGGL((tacc_kernel<rptscene::kTaccReproject>), grid, wg, 0, st, args, px, g, pg, ph, pp, o, h); break;
    }
    return hipGetLastError();
}

}  // namespace rptlaunch
