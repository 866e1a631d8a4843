// vdi_view.hip -- novel-view rendering of a VDI for gfx950.
//
// view_build_kernel: any VDI the context holds (a generator sub-VDI, the gathered composited VDI, an
// uploaded reference-layout VDI) -> the view layout (ViewVdi): per-pixel counts, lists contiguous per pixel
// in y-major rows, per 8x8-pixel tile the largest count.
// vdi_view_kernel: one lane per output pixel, one wave per 8x8 output tile.  The new camera's ray is walked
// through the generating view's clip space, where every list is an axis-aligned column and every
// supersegment a box (the intent of EfficientVDIRaycast.comp's intersectSupersegment): a two-level DDA over
// (tile, cell), every crossing in closed form from the integer index of its plane, every supersegment
// weighted by adjust_opacity(alpha, world length of the ray inside its box) and blended front to back as
// vdi_flatten_kernel blends.  tests/view_ref/view_ref.c restates it operation for operation.
// The compact view layout: view_build_count_kernel and view_build_fill_kernel build it in two
// passes around the offset passes of vdi_pack.hip, and vdi_view_compact_kernel is vdi_view_kernel with a list's
// first entry at boff[p >> 8] + loc[p] instead of p*S.
#include "insitu_device.h"
#include "insitu_kernels.h"
#include "vdi_view_source.h"

#pragma clang fp contract(off)

namespace insitu {

__global__ __launch_bounds__(256) void view_build_kernel(const ViewSource P, const ViewVdi V) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * 4 + wave;
    if (tile >= V.tiles_x * V.tiles_y) return;   // wave-uniform
    const int ty = tile / V.tiles_x, tx = tile - ty * V.tiles_x;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const int S = V.S, H = V.H;
    int n = 0;
    if (x < V.W && y < H) {
        const size_t o = ((size_t)y * (size_t)V.W + (size_t)x) * (size_t)S;
        const ViewAt at = view_at(P, x, y, H, S);
        const int stored = view_slots(P, 0, x, y, S);
        for (; n < stored; ++n) {
            const size_t e = at.e0 + (size_t)n * at.estride;
            const float2 se = P.dep[e];
            if (se.x == 0.0f) break;
            V.col[o + n] = P.col[e];
            V.dep[o + n] = se;
        }
        V.cnt[(size_t)y * (size_t)V.W + (size_t)x] = (uint8_t)n;
    }
    int m = n;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int v = __shfl_xor(m, o);
        m = v > m ? v : m;
    }
    if (lane == 0) V.tmax[tile] = (uint8_t)m;
}

// The compact layout's build, pass 1: the counts and the tiles' largest count as view_build_kernel
// leaves them, nothing else.
__global__ __launch_bounds__(256) void view_build_count_kernel(const ViewSource P, const ViewVdi V) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * 4 + wave;
    if (tile >= V.tiles_x * V.tiles_y) return;   // wave-uniform
    const int ty = tile / V.tiles_x, tx = tile - ty * V.tiles_x;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const int S = V.S, H = V.H;
    int n = 0;
    if (x < V.W && y < H) {
        const ViewAt at = view_at(P, x, y, H, S);
        const int stored = view_slots(P, 0, x, y, S);
        while (n < stored && P.dep[at.e0 + (size_t)n * at.estride].x != 0.0f) ++n;
        V.cnt[(size_t)y * (size_t)V.W + (size_t)x] = (uint8_t)n;
    }
    int m = n;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int v = __shfl_xor(m, o);
        m = v > m ? v : m;
    }
    if (lane == 0) V.tmax[tile] = (uint8_t)m;
}

// ... pass 2, once the offsets of those counts are known: the first cnt[p] entries of every list, at
// boff[p >> 8] + loc[p]
__global__ __launch_bounds__(256) void view_build_fill_kernel(const ViewSource P, const ViewVdi V) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * 4 + wave;
    if (tile >= V.tiles_x * V.tiles_y) return;   // wave-uniform
    const int ty = tile / V.tiles_x, tx = tile - ty * V.tiles_x;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    if (x >= V.W || y >= V.H) return;
    const size_t p = (size_t)y * (size_t)V.W + (size_t)x;
    const size_t o = (size_t)V.boff[p >> 8] + (size_t)V.loc[p];
    const ViewAt at = view_at(P, x, y, V.H, V.S);
    const int n = (int)V.cnt[p];
    for (int i = 0; i < n; ++i) {
        const size_t e = at.e0 + (size_t)i * at.estride;
        V.col[o + i] = P.col[e];
        V.dep[o + i] = P.dep[e];
    }
}

namespace {
template <class Kernel>
hipError_t launch_build(Kernel kernel, const ViewSource& src, const ViewVdi& dst, hipStream_t s) {
    const int tiles = dst.tiles_x * dst.tiles_y;
    if (tiles <= 0 || dst.S <= 0 || dst.S > 255) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, s, src, dst);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_view_build(const ViewSource& src, const ViewVdi& dst, hipStream_t s) {
    if (dst.loc) return hipErrorInvalidValue;
    return launch_build(view_build_kernel, src, dst, s);
}
hipError_t launch_view_build_count(const ViewSource& src, const ViewVdi& dst, hipStream_t s) {
    return launch_build(view_build_count_kernel, src, dst, s);
}
hipError_t launch_view_build_fill(const ViewSource& src, const ViewVdi& dst, hipStream_t s) {
    if (!dst.loc || !dst.boff) return hipErrorInvalidValue;
    return launch_build(view_build_fill_kernel, src, dst, s);
}

namespace {

// The ray in G's clip space, c(s) = cf + s*d, and the plane a = P*w of one family (a = x, y or z):
// n + s*(-q) = P*c_w(s) - c_a(s), so the ray meets the plane at t = n / q (crossings).
struct Plane {
    float n, q, t;
};
__device__ __forceinline__ Plane plane_of(float P, float ca, float da, float cw, float dw) {
    Plane r;
    r.n = __builtin_fmaf(P, cw, -ca);
    r.q = __builtin_fmaf(-P, dw, da);
    r.t = r.n / r.q;
    return r;
}
// [lo, hi] cut to c_a >= P*c_w; hi = -1 empties it (lo >= 0 always)
__device__ __forceinline__ void clip_ge(const Plane& p, float& lo, float& hi) {
    if (p.q > 0.0f) lo = gmax(lo, p.t);
    else if (p.q < 0.0f) hi = gmin(hi, p.t);
    else if (p.n > 0.0f) hi = -1.0f;
}
// ... to c_a <= P*c_w
__device__ __forceinline__ void clip_le(const Plane& p, float& lo, float& hi) {
    if (p.q > 0.0f) hi = gmin(hi, p.t);
    else if (p.q < 0.0f) lo = gmax(lo, p.t);
    else if (p.n < 0.0f) hi = -1.0f;
}
// ... to c_a < P*c_w (a cell owns its lower edge only)
__device__ __forceinline__ void clip_lt(const Plane& p, float& lo, float& hi) {
    if (p.q > 0.0f) hi = gmin(hi, p.t);
    else if (p.q < 0.0f) lo = gmax(lo, p.t);
    else if (!(p.n > 0.0f)) hi = -1.0f;
}
// lower edge of cell k of an axis of n cells: X(k) = (2k - 1)/n - 1, with rn = 1/n
__device__ __forceinline__ float edge_of(int k, float rn) { return __builtin_fmaf((float)(2 * k - 1), rn, -1.0f); }
// the cell that owns NDC coordinate c / cw, clamped to [k0, k1] (NaN: k0)
__device__ __forceinline__ int cell_of(float c, float cw, float half, int k0, int k1) {
    float kf = __builtin_floorf(__builtin_fmaf(c / cw, half, half + 0.5f));
    if (!(kf >= (float)k0)) kf = (float)k0;
    if (kf > (float)k1) kf = (float)k1;
    return (int)kf;
}

// Is the range just after ra / just before rb on the plane's >= side, as the cuts decide it: exactly when
// clip_ge leaves lo at ra / hi at rb, and exactly when clip_lt does not.
__device__ __forceinline__ bool above_from(const Plane& p, float ra) {
    return (p.q > 0.0f) ? (p.t <= ra) : (p.q < 0.0f) ? (p.t > ra) : !(p.n > 0.0f);
}
__device__ __forceinline__ bool above_upto(const Plane& p, float rb) {
    return (p.q > 0.0f) ? (p.t < rb) : (p.q < 0.0f) ? (p.t >= rb) : !(p.n > 0.0f);
}

struct RayG {
    f4 cf, d;
};

// 2-D DDA over granules of g cells inside granules [gx0, gx1] x [gy0, gy1], from the granule that owns the
// start of [ra, rb] to the one that owns its end: every granule on the way is handed to `visit` with the part of
// [ra, rb] inside its four planes (when not empty).  The next granule is across the exit plane met first, the x
// plane on a tie.  (ix, iy) and (ex, ey) are where cell_of puts the two ends; the owner is that granule or, when
// its own lower plane has the point below it or its upper plane has it above, the neighbour across that plane.
template <class Visit>
__device__ __forceinline__ void dda(const RayG& r, float ra, float rb, int g, int W, int H, float rw, float rh, int ix,
                                    int iy, int ex, int ey, int gx0, int gx1, int gy0, int gy1, Visit&& visit) {
    // the planes of granule i of an axis of n cells: its lower edge, cell i*g, and its upper edge, cell
    // min((i + 1)*g, n).  A plane is a function of its cell index alone, so a step carries the plane it
    // crosses over to the next granule instead of computing it again
    auto x_plane = [&](int i) { const int k = i * g; return plane_of(edge_of(k < W ? k : W, rw), r.cf.x, r.d.x, r.cf.w, r.d.w); };
    auto y_plane = [&](int i) { const int k = i * g; return plane_of(edge_of(k < H ? k : H, rh), r.cf.y, r.d.y, r.cf.w, r.d.w); };
    Plane xl = x_plane(ix), xh = x_plane(ix + 1), yl = y_plane(iy), yh = y_plane(iy + 1);
    if (ix > gx0 && !above_from(xl, ra)) { ix -= 1; xh = xl; xl = x_plane(ix); }
    else if (ix < gx1 && above_from(xh, ra)) { ix += 1; xl = xh; xh = x_plane(ix + 1); }
    if (iy > gy0 && !above_from(yl, ra)) { iy -= 1; yh = yl; yl = y_plane(iy); }
    else if (iy < gy1 && above_from(yh, ra)) { iy += 1; yl = yh; yh = y_plane(iy + 1); }
    if (ex > gx0 && !above_upto(x_plane(ex), rb)) ex -= 1;
    else if (ex < gx1 && above_upto(x_plane(ex + 1), rb)) ex += 1;
    if (ey > gy0 && !above_upto(y_plane(ey), rb)) ey -= 1;
    else if (ey < gy1 && above_upto(y_plane(ey + 1), rb)) ey += 1;
    const int sx = ex > ix ? 1 : -1, sy = ey > iy ? 1 : -1;
    for (;;) {
        float lo = ra, hi = rb;
        clip_ge(xl, lo, hi);
        clip_lt(xh, lo, hi);
        clip_ge(yl, lo, hi);
        clip_lt(yh, lo, hi);
        if (hi > lo) visit(ix, iy, lo, hi);
        if (ix == ex && iy == ey) break;
        const float tx = sx > 0 ? xh.t : xl.t, ty = sy > 0 ? yh.t : yl.t;
        if (iy == ey || (ix != ex && tx <= ty)) {
            ix += sx;
            if (sx > 0) { xl = xh; xh = x_plane(ix + 1); }
            else { xh = xl; xl = x_plane(ix); }
        } else {
            iy += sy;
            if (sy > 0) { yl = yh; yh = y_plane(iy + 1); }
            else { yh = yl; yl = y_plane(iy); }
        }
    }
}

// One output pixel's ray through the bound VDI.  COMPACT selects where a list begins (ViewVdi) and nothing else: every
// float operation and its order is the same in both layouts.
template <bool COMPACT>
__device__ __forceinline__ void view_ray(const ViewParams& P) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int otx = (P.out_w + 7) >> 3;
    const int tile = (int)blockIdx.x * 4 + wave;
    const int ox = (tile % otx) * 8 + (lane & 7), oy = (tile / otx) * 8 + (lane >> 3);
    if (ox >= P.out_w || oy >= P.out_h) return;
    const ViewVdi& V = P.vdi;
    const int W = V.W, H = V.H, S = V.S;

    // the new camera's ray (VDIGenerator.comp:305-320) and its end points in G's clip space
    const float uvx = __builtin_fmaf((float)ox / (float)P.out_w, 2.0f, -1.0f);
    const float uvy = __builtin_fmaf((float)oy / (float)P.out_h, 2.0f, -1.0f);
    const f4 wf = persp_div(mat_vec(P.ipv_n, f4{uvx, uvy, -1.0f, 1.0f}));
    const f4 wb = persp_div(mat_vec(P.ipv_n, f4{uvx, uvy, 1.0f, 1.0f}));
    const float L = len4(wb.x - wf.x, wb.y - wf.y, wb.z - wf.z, wb.w - wf.w);
    RayG r;
    r.cf = mat_vec(P.pv_g, wf);
    const f4 cb = mat_vec(P.pv_g, wb);
    r.d = f4{cb.x - r.cf.x, cb.y - r.cf.y, cb.z - r.cf.z, cb.w - r.cf.w};

    float C0 = 0.0f, C1 = 0.0f, C2 = 0.0f, C3 = 0.0f;
    const float rw = 1.0f / (float)W, rh = 1.0f / (float)H;
    // [0, 1] cut to the cells' extent and to -1 <= z <= 1
    float s0 = 0.0f, s1 = 1.0f;
    clip_ge(plane_of(edge_of(0, rw), r.cf.x, r.d.x, r.cf.w, r.d.w), s0, s1);
    clip_lt(plane_of(edge_of(W, rw), r.cf.x, r.d.x, r.cf.w, r.d.w), s0, s1);
    clip_ge(plane_of(edge_of(0, rh), r.cf.y, r.d.y, r.cf.w, r.d.w), s0, s1);
    clip_lt(plane_of(edge_of(H, rh), r.cf.y, r.d.y, r.cf.w, r.d.w), s0, s1);
    clip_ge(plane_of(-1.0f, r.cf.z, r.d.z, r.cf.w, r.d.w), s0, s1);
    clip_le(plane_of(1.0f, r.cf.z, r.d.z, r.cf.w, r.d.w), s0, s1);
    if (s1 > s0) {
        const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
        // the point of the ray at s, as the cell that owns it
        auto cell_x = [&](float s, int k0, int k1) {
            return cell_of(__builtin_fmaf(s, r.d.x, r.cf.x), __builtin_fmaf(s, r.d.w, r.cf.w), hw, k0, k1);
        };
        auto cell_y = [&](float s, int k0, int k1) {
            return cell_of(__builtin_fmaf(s, r.d.y, r.cf.y), __builtin_fmaf(s, r.d.w, r.cf.w), hh, k0, k1);
        };
        // lists are walked backwards when z falls along the ray
        const float z0 = __builtin_fmaf(s0, r.d.z, r.cf.z) / __builtin_fmaf(s0, r.d.w, r.cf.w);
        const float z1 = __builtin_fmaf(s1, r.d.z, r.cf.z) / __builtin_fmaf(s1, r.d.w, r.cf.w);
        const bool back = z1 < z0;
        auto cell = [&](int kx, int ky, float sa, float sb) {
            const size_t p = (size_t)ky * (size_t)W + (size_t)kx;
            const int n = (int)V.cnt[p];
            const size_t at = COMPACT ? (size_t)V.boff[p >> 8] + (size_t)V.loc[p] : p * (size_t)S;
            const float4* col = V.col + at;
            const float2* dep = V.dep + at;
            for (int j = 0; j < n; ++j) {
                const int i = back ? n - 1 - j : j;
                const float2 se = dep[i];
                // the plane the ray leaves the box through is cut first: a box that ends before the cell begins
                // is empty after this cut alone (the other cut could only shrink it further)
                const Plane pl = plane_of(back ? se.x : se.y, r.cf.z, r.d.z, r.cf.w, r.d.w);
                float lo = sa, hi = sb;
                if (back) clip_ge(pl, lo, hi);
                else clip_le(pl, lo, hi);
                if (!(hi > lo)) continue;
                const Plane pf = plane_of(back ? se.y : se.x, r.cf.z, r.d.z, r.cf.w, r.d.w);   // ... enters it through
                if (back) clip_le(pf, lo, hi);
                else clip_ge(pf, lo, hi);
                if (hi > lo) {
                    const float4 c = col[i];
                    const float adj = adjust_opacity(c.w, (hi - lo) * L);
                    const float t = 1.0f - C3;
                    C0 = __builtin_fmaf(t * c.x, adj, C0);
                    C1 = __builtin_fmaf(t * c.y, adj, C1);
                    C2 = __builtin_fmaf(t * c.z, adj, C2);
                    C3 = __builtin_fmaf(t, adj, C3);
                } else if ((back ? pf.q < 0.0f : pf.q > 0.0f) && lo >= sb) {
                    break;   // the box begins at or beyond the cell's end, and so does every later one of the list
                }
            }
        };
        const int kx0 = cell_x(s0, 0, W - 1), ky0 = cell_y(s0, 0, H - 1);
        const int kx1 = cell_x(s1, 0, W - 1), ky1 = cell_y(s1, 0, H - 1);
        dda(r, s0, s1, 8, W, H, rw, rh, kx0 >> 3, ky0 >> 3, kx1 >> 3, ky1 >> 3, 0, (W - 1) >> 3, 0, (H - 1) >> 3,
            [&](int tx, int ty, float ta, float tb) {
            if (P.skip && V.tmax[ty * V.tiles_x + tx] == 0) return;
            const int xa = tx * 8, xb = xa + 7 < W - 1 ? xa + 7 : W - 1;
            const int ya = ty * 8, yb = ya + 7 < H - 1 ? ya + 7 : H - 1;
            dda(r, ta, tb, 1, W, H, rw, rh, cell_x(ta, xa, xb), cell_y(ta, ya, yb), cell_x(tb, xa, xb), cell_y(tb, ya, yb),
                xa, xb, ya, yb, cell);
        });
    }
    const size_t o = (size_t)oy * (size_t)P.out_w + (size_t)ox;
    P.out_color[o] = make_float4(C0, C1, C2, C3);
    P.out_image[o] = unorm8(C0) | (unorm8(C1) << 8) | (unorm8(C2) << 16) | (unorm8(C3) << 24);
}

}  // namespace

__global__ __launch_bounds__(256) void vdi_view_kernel(const ViewParams P) { view_ray<false>(P); }
__global__ __launch_bounds__(256) void vdi_view_compact_kernel(const ViewParams P) { view_ray<true>(P); }

hipError_t launch_vdi_view(const ViewParams& p, hipStream_t s) {
    if (p.out_w <= 0 || p.out_h <= 0) return hipErrorInvalidValue;
    const long long tiles = (long long)((p.out_w + 7) / 8) * (long long)((p.out_h + 7) / 8);
    if (tiles > 0x7fffffffLL / 4) return hipErrorInvalidValue;
    if (p.vdi.loc && !p.vdi.boff) return hipErrorInvalidValue;
    if (p.vdi.loc) hipLaunchKernelGGL(vdi_view_compact_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(vdi_view_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace insitu
