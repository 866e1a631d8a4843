/* view_ref.c -- CPU restatement of novel-view VDI rendering -- TEST INFRASTRUCTURE.
 *
 * Plain C99, one pixel at a time, every float operation in the order section 9 gives it (fmaf only where
 * it is written there).  Built by tests/view_binding.py with the oracle's flags; pow is the contract's
 * orc_pow, taken from liboracle.so.  The GPU kernel (csrc/vdi_view.hip) must equal this bit for bit.
 *
 * The VDI comes in the reference layout: colour (W,H,S,4) rgba32f, depth (W,H,2S) r32f, x slowest.  With
 * `repack` the lists are first copied into the kernel's view layout (counts + y-major contiguous lists) and
 * read from there; without it they are read where they lie.  With `skip` a tile of 8x8 lists that are all
 * empty is stepped over.  Neither may change a bit of the result.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

float orc_pow(float x, float y);   /* liboracle.so */

typedef struct { float x, y, z, w; } v4;

static inline float gmin(float x, float y) { return (y < x) ? y : x; }
static inline float gmax(float x, float y) { return (x < y) ? y : x; }

static inline v4 mat_vec(const float* m, v4 v) {
    v4 r;
    r.x = fmaf(m[12], v.w, fmaf(m[8], v.z, fmaf(m[4], v.y, m[0] * v.x)));
    r.y = fmaf(m[13], v.w, fmaf(m[9], v.z, fmaf(m[5], v.y, m[1] * v.x)));
    r.z = fmaf(m[14], v.w, fmaf(m[10], v.z, fmaf(m[6], v.y, m[2] * v.x)));
    r.w = fmaf(m[15], v.w, fmaf(m[11], v.z, fmaf(m[7], v.y, m[3] * v.x)));
    return r;
}
static inline v4 persp_div(v4 v) {
    float r = 1.0f / v.w;
    v4 o = { v.x * r, v.y * r, v.z * r, v.w * r };
    return o;
}
static inline float len4(float x, float y, float z, float w) {
    return sqrtf(fmaf(w, w, fmaf(z, z, fmaf(y, y, x * x))));
}
static inline float adjust_opacity(float a, float len) { return 1.0f - orc_pow(1.0f - a, len); }
static inline uint8_t unorm8(float x) {
    float q = (x > 0.0f) ? ((x < 1.0f) ? x : 1.0f) : 0.0f;
    return (uint8_t)(int)floorf(fmaf(q, 255.0f, 0.5f));
}

/* the plane a = P*w against the ray c(s) = cf + s*d: met at t = n/q */
typedef struct { float n, q, t; } plane;
static inline plane plane_of(float P, float ca, float da, float cw, float dw) {
    plane r;
    r.n = fmaf(P, cw, -ca);
    r.q = fmaf(-P, dw, da);
    r.t = r.n / r.q;
    return r;
}
/* [lo,hi] cut to c_a >= P c_w / c_a <= P c_w / c_a < P c_w; hi = -1 empties it */
static inline void clip_ge(plane p, float* lo, float* hi) {
    if (p.q > 0.0f) *lo = gmax(*lo, p.t);
    else if (p.q < 0.0f) *hi = gmin(*hi, p.t);
    else if (p.n > 0.0f) *hi = -1.0f;
}
static inline void clip_le(plane p, float* lo, float* hi) {
    if (p.q > 0.0f) *hi = gmin(*hi, p.t);
    else if (p.q < 0.0f) *lo = gmax(*lo, p.t);
    else if (p.n < 0.0f) *hi = -1.0f;
}
static inline void clip_lt(plane p, float* lo, float* hi) {
    if (p.q > 0.0f) *hi = gmin(*hi, p.t);
    else if (p.q < 0.0f) *lo = gmax(*lo, p.t);
    else if (!(p.n > 0.0f)) *hi = -1.0f;
}
static inline float edge_of(int k, float rn) { return fmaf((float)(2 * k - 1), rn, -1.0f); }
static inline int cell_of(float c, float cw, float half, int k0, int k1) {
    float kf = floorf(fmaf(c / cw, half, half + 0.5f));
    if (!(kf >= (float)k0)) kf = (float)k0;
    if (kf > (float)k1) kf = (float)k1;
    return (int)kf;
}
/* is the range just after ra / just before rb on the plane's >= side, as the cuts decide it: exactly when
 * clip_ge leaves lo at ra / hi at rb, and exactly when clip_lt does not */
static inline int above_from(plane p, float ra) {
    return (p.q > 0.0f) ? (p.t <= ra) : (p.q < 0.0f) ? (p.t > ra) : !(p.n > 0.0f);
}
static inline int above_upto(plane p, float rb) {
    return (p.q > 0.0f) ? (p.t < rb) : (p.q < 0.0f) ? (p.t >= rb) : !(p.n > 0.0f);
}

typedef struct {
    /* the lists: reference layout, or (repacked) the view layout */
    const float* color;
    const float* depth;
    const uint8_t* cnt;      /* view layout only */
    const uint8_t* tmax;     /* skip only: per 8x8 tile the largest count */
    int W, H, S, tiles_x, skip;
    /* the ray */
    v4 cf, d;
    float L, rw, rh, hw, hh;
    int back;
    float C[4];
    long long cells, examined, blended;   /* work counters (tools/view_bench.py) */
    /* of the pixel in hand (the partition check): summed length and number of the level-1 and level-2 intervals */
    double cover1, cover2;
    long long n1, n2;
} walk;

static int list_of(const walk* k, int x, int y, const float** col, const float** dep) {
    if (k->cnt) {
        size_t p = (size_t)y * (size_t)k->W + (size_t)x;
        *col = k->color + p * (size_t)k->S * 4;
        *dep = k->depth + p * (size_t)k->S * 2;
        return (int)k->cnt[p];
    }
    size_t p = (size_t)x * (size_t)k->H + (size_t)y;
    *col = k->color + p * (size_t)k->S * 4;
    *dep = k->depth + p * (size_t)k->S * 2;
    int n = 0;
    while (n < k->S && (*dep)[2 * n] != 0.0f) ++n;
    return n;
}

static void visit_cell(walk* k, int kx, int ky, float sa, float sb) {
    const float *col, *dep;
    int n = list_of(k, kx, ky, &col, &dep);
    k->cells += 1;
    for (int j = 0; j < n; ++j) {
        int i = k->back ? n - 1 - j : j;
        k->examined += 1;
        /* the list in walking order: the plane the ray leaves the box through is cut first (a box that ends
         * before the cell begins is empty after it), then the plane it enters through */
        plane pl = plane_of(k->back ? dep[2 * i] : dep[2 * i + 1], k->cf.z, k->d.z, k->cf.w, k->d.w);
        float lo = sa, hi = sb;
        if (k->back) clip_ge(pl, &lo, &hi);
        else clip_le(pl, &lo, &hi);
        if (!(hi > lo)) continue;
        plane pf = plane_of(k->back ? dep[2 * i + 1] : dep[2 * i], k->cf.z, k->d.z, k->cf.w, k->d.w);
        if (k->back) clip_le(pf, &lo, &hi);
        else clip_ge(pf, &lo, &hi);
        if (hi > lo) {
            k->blended += 1;
            const float* c = col + 4 * i;
            float adj = adjust_opacity(c[3], (hi - lo) * k->L);
            float t = 1.0f - k->C[3];
            k->C[0] = fmaf(t * c[0], adj, k->C[0]);
            k->C[1] = fmaf(t * c[1], adj, k->C[1]);
            k->C[2] = fmaf(t * c[2], adj, k->C[2]);
            k->C[3] = fmaf(t, adj, k->C[3]);
        } else if ((k->back ? pf.q < 0.0f : pf.q > 0.0f) && lo >= sb) {
            break;   /* begins at or beyond the cell's end: so does every later entry of an ordered list */
        }
    }
}

static inline int cell_x(const walk* k, float s, int k0, int k1) {
    return cell_of(fmaf(s, k->d.x, k->cf.x), fmaf(s, k->d.w, k->cf.w), k->hw, k0, k1);
}
static inline int cell_y(const walk* k, float s, int k0, int k1) {
    return cell_of(fmaf(s, k->d.y, k->cf.y), fmaf(s, k->d.w, k->cf.w), k->hh, k0, k1);
}

/* plane i of the granules of g cells along x / y: the lower edge of cell min(i*g, n) */
static inline plane x_plane(const walk* k, int i, int g) {
    int c = i * g;
    return plane_of(edge_of(c < k->W ? c : k->W, k->rw), k->cf.x, k->d.x, k->cf.w, k->d.w);
}
static inline plane y_plane(const walk* k, int i, int g) {
    int c = i * g;
    return plane_of(edge_of(c < k->H ? c : k->H, k->rh), k->cf.y, k->d.y, k->cf.w, k->d.w);
}
/* the granule of [i0, i1] that owns the start (end = 0) or the end (end = 1) of the range by the cuts: i, or
 * its neighbour when i's own lower plane has the point below it or its upper plane has it above */
static inline int own_x(const walk* k, int g, int i, int i0, int i1, float s, int end) {
    if (i > i0) { plane p = x_plane(k, i, g); if (!(end ? above_upto(p, s) : above_from(p, s))) return i - 1; }
    if (i < i1) { plane p = x_plane(k, i + 1, g); if (end ? above_upto(p, s) : above_from(p, s)) return i + 1; }
    return i;
}
static inline int own_y(const walk* k, int g, int i, int i0, int i1, float s, int end) {
    if (i > i0) { plane p = y_plane(k, i, g); if (!(end ? above_upto(p, s) : above_from(p, s))) return i - 1; }
    if (i < i1) { plane p = y_plane(k, i + 1, g); if (end ? above_upto(p, s) : above_from(p, s)) return i + 1; }
    return i;
}

/* the 2-D DDA of section 9 over granules of g cells (8: tiles, 1: cells) inside granules [gx0, gx1] x [gy0, gy1];
 * (ix, iy) and (ex, ey) are where cell_of puts the ends of [ra, rb], corrected here to the granules that own them */
static void dda(walk* k, float ra, float rb, int g, int ix, int iy, int ex, int ey, int gx0, int gx1, int gy0, int gy1) {
    ix = own_x(k, g, ix, gx0, gx1, ra, 0);
    iy = own_y(k, g, iy, gy0, gy1, ra, 0);
    ex = own_x(k, g, ex, gx0, gx1, rb, 1);
    ey = own_y(k, g, ey, gy0, gy1, rb, 1);
    const int sx = ex > ix ? 1 : -1, sy = ey > iy ? 1 : -1;
    for (;;) {
        plane xl = x_plane(k, ix, g), xh = x_plane(k, ix + 1, g);
        plane yl = y_plane(k, iy, g), yh = y_plane(k, iy + 1, g);
        float lo = ra, hi = rb;
        clip_ge(xl, &lo, &hi);
        clip_lt(xh, &lo, &hi);
        clip_ge(yl, &lo, &hi);
        clip_lt(yh, &lo, &hi);
        if (hi > lo) {
            if (g == 1) {
                k->cover2 += (double)hi - (double)lo;
                k->n2 += 1;
                visit_cell(k, ix, iy, lo, hi);
            } else {
                k->cover1 += (double)hi - (double)lo;
                k->n1 += 1;
                if (!(k->skip && k->tmax[iy * k->tiles_x + ix] == 0)) {
                    const int W = k->W, H = k->H;
                    int xa = ix * 8, xb = xa + 7 < W - 1 ? xa + 7 : W - 1;
                    int ya = iy * 8, yb = ya + 7 < H - 1 ? ya + 7 : H - 1;
                    dda(k, lo, hi, 1, cell_x(k, lo, xa, xb), cell_y(k, lo, ya, yb), cell_x(k, hi, xa, xb),
                        cell_y(k, hi, ya, yb), xa, xb, ya, yb);
                }
            }
        }
        if (ix == ex && iy == ey) break;
        float tx = sx > 0 ? xh.t : xl.t, ty = sy > 0 ? yh.t : yl.t;
        if (iy == ey || (ix != ex && tx <= ty)) ix += sx;
        else iy += sy;
    }
}

/* returns s1 - s0, the part of the ray inside the cells' extent (0 when nothing is left) */
static float view_pixel(walk* k, const float* pv_g, const float* ipv_n, int ox, int oy, int out_w, int out_h) {
    float uvx = fmaf((float)ox / (float)out_w, 2.0f, -1.0f);
    float uvy = fmaf((float)oy / (float)out_h, 2.0f, -1.0f);
    v4 front = { uvx, uvy, -1.0f, 1.0f }, backp = { uvx, uvy, 1.0f, 1.0f };
    v4 wf = persp_div(mat_vec(ipv_n, front));
    v4 wb = persp_div(mat_vec(ipv_n, backp));
    k->L = len4(wb.x - wf.x, wb.y - wf.y, wb.z - wf.z, wb.w - wf.w);
    k->cf = mat_vec(pv_g, wf);
    v4 cb = mat_vec(pv_g, wb);
    k->d.x = cb.x - k->cf.x; k->d.y = cb.y - k->cf.y; k->d.z = cb.z - k->cf.z; k->d.w = cb.w - k->cf.w;
    k->C[0] = k->C[1] = k->C[2] = k->C[3] = 0.0f;
    k->cover1 = k->cover2 = 0.0;
    k->n1 = k->n2 = 0;
    const int W = k->W, H = k->H;
    float s0 = 0.0f, s1 = 1.0f;
    clip_ge(plane_of(edge_of(0, k->rw), k->cf.x, k->d.x, k->cf.w, k->d.w), &s0, &s1);
    clip_lt(plane_of(edge_of(W, k->rw), k->cf.x, k->d.x, k->cf.w, k->d.w), &s0, &s1);
    clip_ge(plane_of(edge_of(0, k->rh), k->cf.y, k->d.y, k->cf.w, k->d.w), &s0, &s1);
    clip_lt(plane_of(edge_of(H, k->rh), k->cf.y, k->d.y, k->cf.w, k->d.w), &s0, &s1);
    clip_ge(plane_of(-1.0f, k->cf.z, k->d.z, k->cf.w, k->d.w), &s0, &s1);
    clip_le(plane_of(1.0f, k->cf.z, k->d.z, k->cf.w, k->d.w), &s0, &s1);
    if (!(s1 > s0)) return 0.0f;
    float z0 = fmaf(s0, k->d.z, k->cf.z) / fmaf(s0, k->d.w, k->cf.w);
    float z1 = fmaf(s1, k->d.z, k->cf.z) / fmaf(s1, k->d.w, k->cf.w);
    k->back = z1 < z0;
    int kx0 = cell_x(k, s0, 0, W - 1), ky0 = cell_y(k, s0, 0, H - 1);
    int kx1 = cell_x(k, s1, 0, W - 1), ky1 = cell_y(k, s1, 0, H - 1);
    dda(k, s0, s1, 8, kx0 >> 3, ky0 >> 3, kx1 >> 3, ky1 >> 3, 0, (W - 1) >> 3, 0, (H - 1) >> 3);
    return s1 - s0;
}

/* out_color: (out_h, out_w, 4) float; out_image: (out_h, out_w, 4) uint8; work (may be NULL): cells visited,
 * list entries examined in them, entries blended, over all rays; part (may be NULL): (out_h, out_w, 5) double,
 * per pixel s1 - s0, the summed length (each hi - lo in double) and the number of the level-1 intervals
 * visited, and the same two of the level-2 intervals.  0 on success. */
int view_ref_render(const float* color, const float* depth, int W, int H, int S, const float* pv_g,
                    const float* ipv_n, int out_w, int out_h, int skip, int repack, float* out_color,
                    uint8_t* out_image, long long* work, double* part) {
    if (!color || !depth || !pv_g || !ipv_n || !out_color || !out_image) return -1;
    if (W <= 0 || H <= 0 || S <= 0 || S > 255 || out_w <= 0 || out_h <= 0) return -1;
    const int tiles_x = (W + 7) / 8, tiles_y = (H + 7) / 8;
    const size_t px = (size_t)W * (size_t)H;
    uint8_t* tmax = NULL;
    uint8_t* cnt = NULL;
    float* vcol = NULL;
    float* vdep = NULL;
    if (skip || repack) {
        tmax = (uint8_t*)calloc((size_t)tiles_x * (size_t)tiles_y, 1);
        if (!tmax) return -2;
    }
    if (repack) {
        cnt = (uint8_t*)calloc(px, 1);
        vcol = (float*)calloc(px * (size_t)S * 4, sizeof(float));
        vdep = (float*)calloc(px * (size_t)S * 2, sizeof(float));
        if (!cnt || !vcol || !vdep) { free(tmax); free(cnt); free(vcol); free(vdep); return -2; }
    }
    if (tmax) {
        for (int x = 0; x < W; ++x) {
            for (int y = 0; y < H; ++y) {
                size_t r = ((size_t)x * (size_t)H + (size_t)y) * (size_t)S;
                int n = 0;
                while (n < S && depth[2 * (r + n)] != 0.0f) ++n;
                uint8_t* t = &tmax[(y >> 3) * tiles_x + (x >> 3)];
                if (n > *t) *t = (uint8_t)n;
                if (repack) {
                    size_t p = (size_t)y * (size_t)W + (size_t)x;
                    cnt[p] = (uint8_t)n;
                    memcpy(vcol + p * (size_t)S * 4, color + r * 4, (size_t)n * 16);
                    memcpy(vdep + p * (size_t)S * 2, depth + r * 2, (size_t)n * 8);
                }
            }
        }
    }
    long long cells = 0, examined = 0, blended = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : cells, examined, blended)
    for (int oy = 0; oy < out_h; ++oy) {
        walk k;
        memset(&k, 0, sizeof k);
        k.color = repack ? vcol : color;
        k.depth = repack ? vdep : depth;
        k.cnt = cnt;
        k.tmax = tmax;
        k.W = W; k.H = H; k.S = S; k.tiles_x = tiles_x; k.skip = skip;
        k.rw = 1.0f / (float)W; k.rh = 1.0f / (float)H;
        k.hw = 0.5f * (float)W; k.hh = 0.5f * (float)H;
        for (int ox = 0; ox < out_w; ++ox) {
            float span = view_pixel(&k, pv_g, ipv_n, ox, oy, out_w, out_h);
            size_t o = ((size_t)oy * (size_t)out_w + (size_t)ox) * 4;
            if (part) {
                double* pp = part + ((size_t)oy * (size_t)out_w + (size_t)ox) * 5;
                pp[0] = (double)span;
                pp[1] = k.cover1; pp[2] = (double)k.n1;
                pp[3] = k.cover2; pp[4] = (double)k.n2;
            }
            for (int c = 0; c < 4; ++c) {
                out_color[o + c] = k.C[c];
                out_image[o + c] = unorm8(k.C[c]);
            }
        }
        cells += k.cells; examined += k.examined; blended += k.blended;
    }
    if (work) { work[0] = cells; work[1] = examined; work[2] = blended; }
    free(tmax); free(cnt); free(vcol); free(vdep);
    return 0;
}
