// depth_views.hip -- SimpleView's depth rasteriser: `PCViews.get_img` -> `points2depth` -> `distribute`
// (openpoints/models/backbone/simpleview_util.py:60-171, 235-292) as ONE forward launch and ONE backward launch.
//
//   forward    points (B,N,3), rot (V,3,3), trans (V,3) -> img (B*V,H,W), sw (B*V,H,W); image b*V + v is cloud b under view v
//   transform  q_c = ((p0 * R[0][c] + p1 * R[1][c]) + p2 * R[2][c]) - t[c]      fp32, no fma (the library is built with
//              -ffp-contract=off); rot == nullptr: the points are camera-frame already (q = p, V = 1)
//   project    cx = (x / (z + 1e-12f)) * (float)((double)W / H),  cy = y / (z + 1e-12f)
//              _x = ((cx + 1) * H) / 2,  _y = ((cy + 1) * W) / 2
//              ex = ceil(_x + oi), ey = ceil(_y + oj);  oi = i - sx/2 (sx > 1) or -0.5 (sx = 1), i < sx; oj likewise
//              valid = 0 <= ex <= H-1 and 0 <= ey <= W-1 and 0 <= z < inf;   pixel = ex * W + ey   (ex is the ROW)
//              w = 1 / (z + 1e-12f),  wv = z * w
//   sums       per pixel, sw = sum w and sv = sum wv over its valid splats in ascending (point, i, j) order, from +0
//   finish     sw' = sw + (sw == 0),  img = sv / sw';  a pixel without a splat: img = sw = 0
//
// How: a workgroup per image.  Every splat's key `pixel << lg | splat` (lg = log2 of the padded splat count; invalid
// splats and padding: DV_PAD) goes to LDS with the point's depth beside it, the keys are sorted (lds_bitonic.h: a fixed
// network), and the thread that finds a run's head walks the run -- ascending splat = ascending (point, i, j) -- and writes
// the pixel.  An LDS bitmap of the touched pixels (integer OR: order-free) tells the zero pass which pixels are left to
// it, so every element of img and sw is written exactly once and nothing has to arrive zeroed.  No float atomic, no
// memset, no global scratch: the outputs are a pure function of the inputs.
//
//   backward   g (B*V,H,W) -> dpoints (B,N,3): the thread that owns a point recomputes its V*sx*sy splats with the code
//              above (one function: the same pixels), gathers g, img and sw at each and adds, per view,
//                  a = g / sw',  gw = -(a * img),  gz += a * w - (a * z + gw) * (w * w)
//              (what autograd forms for wv = z * w, w = 1 / (z + eps), img = sv / sw'), then
//                  dpoints[k] += gz * R_v[k][2]                       views ascending, splats (i, j) ascending inside
//              The pixel coordinates pass through ceil: the camera frame's x and y get exactly zero (rot == nullptr:
//              dpoints = (0, 0, gz)).  One owner per output element.
//
// Non-finite coordinates (the reference is unspecified there) fail the comparisons above: they contribute nothing and
// index nothing.
#include "apn_common.h"
#include "lds_bitonic.h"

namespace apn {

// what the design holds: the keys of one image in LDS (4 B each, padded to a power of two), the depths of its points
// (4 B each) and one bit per pixel -- 64 + 64 + 8 KiB at the bounds, of the 160 KiB a workgroup may declare
constexpr int DV_THREADS = 1024;
constexpr int DV_MAX_SPLATS = 16384;        // N * sx * sy
constexpr int DV_MAX_PIXELS = 65536;        // H * W; pixel << 14 | splat stays below 2^30
constexpr int DV_MAX_VIEWS = 64;
constexpr int DV_MAX_IMAGES = (1 << 22) - 1;  // B * V: a grid of that many workgroups of DV_THREADS stays below 2^32 threads
constexpr int DV_MAX_LDS = (2 * DV_MAX_SPLATS + DV_MAX_PIXELS / 32) * 4;
constexpr unsigned DV_PAD = 0xFFFFFFFFu;
constexpr float DV_EPS = 1e-12f;

struct DvGeom {
    int h, w, lsx, lsy;                     // splat sizes as log2: sx, sy in {1, 2, 4}
    float aspect;                           // (float)((double)w / h)
};

__device__ __forceinline__ float3 dv_transform(const float *p, const float *rot, const float *trans) {
    const float p0 = p[0], p1 = p[1], p2 = p[2];
    if (rot == nullptr) return make_float3(p0, p1, p2);
    float3 q;
    q.x = ((p0 * rot[0] + p1 * rot[3]) + p2 * rot[6]) - trans[0];
    q.y = ((p0 * rot[1] + p1 * rot[4]) + p2 * rot[7]) - trans[1];
    q.z = ((p0 * rot[2] + p1 * rot[5]) + p2 * rot[8]) - trans[2];
    return q;
}

// the continuous image coordinates of a camera-frame point
__device__ __forceinline__ void dv_project(const DvGeom &g, float3 q, float &fx, float &fy) {
    const float d = q.z + DV_EPS;
    const float cx = (q.x / d) * g.aspect, cy = q.y / d;
    fx = ((cx + 1.0f) * (float)g.h) / 2.0f;
    fy = ((cy + 1.0f) * (float)g.w) / 2.0f;
}

// splat (i, j) of a point at (fx, fy) with depth z: its pixel, or -1
__device__ __forceinline__ int dv_pixel(const DvGeom &g, float fx, float fy, float z, int i, int j) {
    const float oi = g.lsx ? (float)(i - (1 << (g.lsx - 1))) : -0.5f;
    const float oj = g.lsy ? (float)(j - (1 << (g.lsy - 1))) : -0.5f;
    const float ex = __builtin_ceilf(fx + oi), ey = __builtin_ceilf(fy + oj);
    const bool ok = ex >= 0.0f && ex <= (float)(g.h - 1) && ey >= 0.0f && ey <= (float)(g.w - 1) && z >= 0.0f &&
                    z <= 3.402823466e+38f;
    return ok ? (int)ex * g.w + (int)ey : -1;
}

// P: the padded splat count (a power of two >= n << (lsx + lsy)), lg = log2 P.  Dynamic LDS: P keys, n depths,
// (h*w + 31) / 32 bitmap words.
__global__ __launch_bounds__(DV_THREADS) void dv_fwd_kernel(int n, int views, DvGeom g, int P, int lg, const float *points,
                                                             const float *rot, const float *trans, float *img, float *sw_out) {
    extern __shared__ unsigned dv_lds[];
    unsigned *keys = dv_lds;
    float *zs = (float *)(dv_lds + P);
    unsigned *bits = dv_lds + P + n;
    const int t = threadIdx.x;
    const int image = blockIdx.x, cloud = image / views, view = image - cloud * views;
    const int hw = g.h * g.w, words = (hw + 31) >> 5, ls = g.lsx + g.lsy, splats = n << ls;
    const float *R = rot ? rot + 9 * view : nullptr, *T = rot ? trans + 3 * view : nullptr;
    const float *pts = points + (size_t)cloud * n * 3;
    for (int k = t; k < words; k += DV_THREADS) bits[k] = 0u;
    __syncthreads();
    for (int k = t; k < P; k += DV_THREADS) {
        unsigned key = DV_PAD;
        if (k < splats) {
            const int pt = k >> ls, ij = k & ((1 << ls) - 1);
            const float3 q = dv_transform(pts + 3 * pt, R, T);
            float fx, fy;
            dv_project(g, q, fx, fy);
            if (ij == 0) zs[pt] = q.z;
            const int pix = dv_pixel(g, fx, fy, q.z, ij >> g.lsy, ij & ((1 << g.lsy) - 1));
            if (pix >= 0) {
                key = ((unsigned)pix << lg) | (unsigned)k;
                atomicOr(&bits[pix >> 5], 1u << (pix & 31));
            }
        }
        keys[k] = key;
    }
    __syncthreads();
    lds_bitonic_sort<DV_THREADS>(keys, P);
    float *im = img + (size_t)image * hw, *so = sw_out + (size_t)image * hw;
    for (int k = t; k < P; k += DV_THREADS) {
        const unsigned key = keys[k];
        if (key == DV_PAD) continue;
        const unsigned pix = key >> lg;
        if (k > 0 && (keys[k - 1] >> lg) == pix) continue;          // not a run's head
        float sw = 0.0f, sv = 0.0f;
        for (int m = k; m < P; ++m) {
            const unsigned km = keys[m];
            if (km == DV_PAD || (km >> lg) != pix) break;
            const float z = zs[(km & ((1u << lg) - 1u)) >> ls];
            const float w = 1.0f / (z + DV_EPS);
            sw = sw + w;
            sv = sv + z * w;
        }
        so[pix] = sw;
        im[pix] = sv / (sw + (sw == 0.0f ? 1.0f : 0.0f));
    }
    for (int p = t; p < hw; p += DV_THREADS)
        if (!((bits[p >> 5] >> (p & 31)) & 1u)) {
            im[p] = 0.0f;
            so[p] = 0.0f;
        }
}

__global__ __launch_bounds__(256) void dv_bwd_kernel(long long total, int n, int views, DvGeom g, const float *points,
                                                     const float *rot, const float *trans, const float *gout,
                                                     const float *img, const float *sw_in, float *dpoints) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const long long cloud = id / n;
    const int hw = g.h * g.w, sx = 1 << g.lsx, sy = 1 << g.lsy;
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
    for (int v = 0; v < views; ++v) {
        const float *R = rot ? rot + 9 * v : nullptr, *T = rot ? trans + 3 * v : nullptr;
        const float3 q = dv_transform(points + 3 * id, R, T);
        float fx, fy;
        dv_project(g, q, fx, fy);
        const float w = 1.0f / (q.z + DV_EPS);
        const size_t base = (size_t)(cloud * views + v) * hw;
        float gz = 0.0f;
        for (int i = 0; i < sx; ++i)
            for (int j = 0; j < sy; ++j) {
                const int pix = dv_pixel(g, fx, fy, q.z, i, j);
                if (pix < 0) continue;
                const float sw = sw_in[base + pix];
                const float a = gout[base + pix] / (sw + (sw == 0.0f ? 1.0f : 0.0f));
                const float gw = -(a * img[base + pix]);
                gz = gz + (a * w - (a * q.z + gw) * (w * w));
            }
        if (R) {
            d0 = d0 + gz * R[2];
            d1 = d1 + gz * R[5];
            d2 = d2 + gz * R[8];
        } else {
            d2 = d2 + gz;
        }
    }
    dpoints[3 * id] = d0;
    dpoints[3 * id + 1] = d1;
    dpoints[3 * id + 2] = d2;
}

static int dv_log2(int s) { return s == 1 ? 0 : s == 2 ? 1 : s == 4 ? 2 : -1; }

// -> APN_OK with the geometry filled in, or APN_EINVAL
static int dv_check(int b, int n, int views, int h, int w, int sx, int sy, bool has_rot, DvGeom *g) {
    const int lsx = dv_log2(sx), lsy = dv_log2(sy);
    if (lsx < 0 || lsy < 0 || b <= 0 || n <= 0 || views <= 0 || h <= 0 || w <= 0) return APN_EINVAL;
    if (views > DV_MAX_VIEWS || (!has_rot && views != 1)) return APN_EINVAL;
    if ((long long)h * w > DV_MAX_PIXELS || ((long long)n << (lsx + lsy)) > DV_MAX_SPLATS) return APN_EINVAL;
    if ((long long)b * views > DV_MAX_IMAGES || (long long)b * n > 0x7fffffffLL) return APN_EINVAL;     // grids
    g->h = h, g->w = w, g->lsx = lsx, g->lsy = lsy;
    g->aspect = (float)((double)w / (double)h);
    return APN_OK;
}

static DynLdsOnce dv_lds_once;

}  // namespace apn

extern "C" int apn_depth_views_max_splats(void) { return apn::DV_MAX_SPLATS; }
extern "C" int apn_depth_views_max_pixels(void) { return apn::DV_MAX_PIXELS; }
extern "C" int apn_depth_views_max_views(void) { return apn::DV_MAX_VIEWS; }
extern "C" int apn_depth_views_max_images(void) { return apn::DV_MAX_IMAGES; }

extern "C" int apn_depth_views_fwd(int b, int n, int views, int h, int w, int sx, int sy, const float *points,
                                   const float *rot, const float *trans, float *img, float *sw, void *stream) {
    using namespace apn;
    DvGeom g;
    if (int e = dv_check(b, n, views, h, w, sx, sy, rot != nullptr, &g)) return e;
    if (!points || !img || !sw || (rot && !trans)) return APN_EINVAL;
    const int splats = n << (g.lsx + g.lsy);
    int P = 1, lg = 0;
    while (P < splats) P <<= 1, ++lg;
    const int bytes = (P + n + (h * w + 31) / 32) * 4;
    if (hipError_t e = set_dyn_lds(dv_lds_once, (const void *)dv_fwd_kernel, DV_MAX_LDS)) return (int)e;
    hipLaunchKernelGGL(dv_fwd_kernel, dim3(b * views), dim3(DV_THREADS), bytes, (hipStream_t)stream, n, views, g, P, lg,
                       points, rot, trans, img, sw);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_depth_views_bwd(int b, int n, int views, int h, int w, int sx, int sy, const float *points,
                                   const float *rot, const float *trans, const float *g_img, const float *img,
                                   const float *sw, float *dpoints, void *stream) {
    using namespace apn;
    DvGeom g;
    if (int e = dv_check(b, n, views, h, w, sx, sy, rot != nullptr, &g)) return e;
    if (!points || !g_img || !img || !sw || !dpoints || (rot && !trans)) return APN_EINVAL;
    const long long total = (long long)b * n;
    hipLaunchKernelGGL(dv_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, total, n,
                       views, g, points, rot, trans, g_img, img, sw, dpoints);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
