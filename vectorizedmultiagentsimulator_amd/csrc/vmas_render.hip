// vmas_render.hip -- rgb_array rendering: a rasteriser over primitive tables (vmas_render_frames)
// and the kernel that builds the entity layer of such a table, and the camera, from the state
// tensors of a batch (vmas_render_scene).  The frame function is stated in include/vmas_mi355x.h;
// the device kernels and the host backend below evaluate the SAME __host__ __device__ code, in fp32
// with separate roundings (-ffp-contract=off holds for both passes of this file).
//
// k_render_frames: one workgroup per 16 x 16 tile of one frame, one thread per pixel.  The frame's
// table is taken in chunks of 256 records: thread t looks at record base + t, keeps it when its
// bounding box touches the tile, and the kept records are compacted IN TABLE ORDER into LDS (64-bit
// __ballot + popcount prefix inside a wave, the four waves' counts through LDS), so every thread
// then composites the same short list with wave-uniform LDS reads.  The colour lives in three
// registers; the tile's 768 bytes are staged in LDS and leave as whole dwords when the frame width
// is a multiple of 4 (every row then starts on a dword), as bytes otherwise.  No atomics, nothing
// shared between workgroups.  Store-bound at best: E * H * W * 3 bytes written once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "vmas_aux.hpp"
#include "vmas_mi355x.h"

namespace {

#define VR_HD __host__ __device__ __forceinline__

constexpr int kTile = 16, kThreads = kTile * kTile, kChunk = kThreads;
constexpr float kFar = 1e30f;

VR_HD float seg_dist(float qx, float qy, float ax, float ay, float bx, float by) {
    const float ex = bx - ax, ey = by - ay, px = qx - ax, py = qy - ay;
    const float ee = ex * ex + ey * ey;
    float t = ee > 0.0f ? (px * ex + py * ey) / ee : 0.0f;
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const float dx = px - t * ex, dy = py - t * ey;
    return sqrtf(dx * dx + dy * dy);
}

VR_HD float line_width(float w) { return w < 1.0f ? 1.0f : w; }

// distance along one axis to the nearest grid line: lines at m * sp, m = lo..hi, from the line
// nearest the grid's origin (small numbers near the frame: the rounding stays near 1e-5 pixels)
VR_HD float grid_axis(float u, float sp, float lo, float hi) {
    float m = floorf(u / sp + 0.5f);
    m = fminf(fmaxf(m, lo), hi);
    return fabsf(u - m * sp);
}

VR_HD float prim_distance(const VmasRenderPrim& pr, const float* __restrict__ verts, float qx, float qy) {
    switch (pr.kind) {
    case VMAS_PRIM_DISC: {
        const float dx = qx - pr.p[0], dy = qy - pr.p[1];
        return sqrtf(dx * dx + dy * dy) - pr.p[2];
    }
    case VMAS_PRIM_RING: {
        const float dx = qx - pr.p[0], dy = qy - pr.p[1];
        return fabsf(sqrtf(dx * dx + dy * dy) - pr.p[2]) - 0.5f * line_width(pr.p[3]);
    }
    case VMAS_PRIM_SEG:
        return seg_dist(qx, qy, pr.p[0], pr.p[1], pr.p[2], pr.p[3]) - 0.5f * line_width(pr.p[4]);
    case VMAS_PRIM_GRID: {
        const float ux = qx - pr.p[0], uy = qy - pr.p[1], half = pr.p[3];
        if (fabsf(ux) > half || fabsf(uy) > half) return kFar;
        const float lo = (float)pr.v0, hi = (float)pr.nv;
        const float dx = grid_axis(ux - pr.p[5], pr.p[2], lo, hi), dy = grid_axis(uy - pr.p[5], pr.p[2], lo, hi);
        return fminf(dx, dy) - 0.5f * line_width(pr.p[4]);
    }
    case VMAS_PRIM_POLY: {
        const float* v = verts + 2 * (int64_t)pr.v0;
        float best = kFar;
        bool inside = false;
        float xj = v[2 * (pr.nv - 1)], yj = v[2 * (pr.nv - 1) + 1];
        for (int i = 0; i < pr.nv; ++i) {
            const float xi = v[2 * i], yi = v[2 * i + 1];
            best = fminf(best, seg_dist(qx, qy, xj, yj, xi, yi));
            if ((yi > qy) != (yj > qy)) {
                const float xc = (xj - xi) * (qy - yi) / (yj - yi) + xi;
                if (qx < xc) inside = !inside;
            }
            xj = xi;
            yj = yi;
        }
        return inside ? -best : best;
    }
    default:
        return kFar;
    }
}

VR_HD void blend(float& r, float& g, float& b, float cr, float cg, float cb, float a, float d) {
    const float cov = fminf(fmaxf(0.5f - d, 0.0f), 1.0f);
    const float w = a * cov, k = 1.0f - w;
    r = r * k + cr * w;
    g = g * k + cg * w;
    b = b * k + cb * w;
}

VR_HD void composite(const VmasRenderPrim& pr, const float* __restrict__ verts, float qx, float qy, float& r, float& g,
                     float& b) {
    const float d = prim_distance(pr, verts, qx, qy);
    blend(r, g, b, pr.rgba[0], pr.rgba[1], pr.rgba[2], pr.rgba[3], d);
    if ((pr.flags & VMAS_PRIM_BORDER) && (pr.kind == VMAS_PRIM_DISC || pr.kind == VMAS_PRIM_POLY))
        blend(r, g, b, 0.5f * pr.rgba[0], 0.5f * pr.rgba[1], 0.5f * pr.rgba[2], 0.5f * pr.rgba[3], fabsf(d) - 1.0f);
}

VR_HD uint32_t to_byte(float c) { return (uint32_t)floorf(255.0f * c + 0.5f); }

__global__ void __launch_bounds__(kThreads)
k_render_frames(const VmasRenderPrim* __restrict__ prims, int n_prims, const float* __restrict__ verts,
                int n_verts, uint8_t* __restrict__ out, int H, int W, int tiles_x, int tiles_per_frame, int dwords) {
    __shared__ VmasRenderPrim s_prim[kChunk];
    __shared__ int s_wave[kThreads / 64];
    __shared__ uint32_t s_out[kThreads * 3 / 4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frame = (int)(blockIdx.x / (unsigned)tiles_per_frame);
    const int tile = (int)(blockIdx.x % (unsigned)tiles_per_frame);
    const int ty = tile / tiles_x, tx = tile % tiles_x;
    const int i = ty * kTile + (tid >> 4), j = tx * kTile + (tid & 15);
    const float qx = (float)j + 0.5f, qy = (float)(H - i) - 0.5f;
    // the tile in pixel space (y up)
    const float x0 = (float)(tx * kTile), x1 = x0 + (float)kTile;
    const float y1 = (float)(H - ty * kTile), y0 = y1 - (float)kTile;
    const VmasRenderPrim* __restrict__ row = prims + (int64_t)frame * n_prims;
    float r = 1.0f, g = 1.0f, b = 1.0f;
    for (int base = 0; base < n_prims; base += kChunk) {
        const int idx = base + tid;
        bool keep = false;
        if (idx < n_prims) {
            const VmasRenderPrim& pr = row[idx];
            keep = pr.kind != VMAS_PRIM_NONE && pr.bbox[0] <= x1 && pr.bbox[2] >= x0 && pr.bbox[1] <= y1 &&
                   pr.bbox[3] >= y0;
            // (a POLY whose vertices are not all in the pool is not drawn: nothing is read past it)
            if (pr.kind == VMAS_PRIM_POLY && (pr.nv < 3 || pr.v0 < 0 || (int64_t)pr.v0 + pr.nv > n_verts)) keep = false;
        }
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            const int c = s_wave[w];
            off += w < wave ? c : 0;
            total += c;
        }
        if (keep) s_prim[off + before] = row[idx];
        __syncthreads();
        for (int k = 0; k < total; ++k) composite(s_prim[k], verts, qx, qy, r, g, b);
        __syncthreads();  // (the next chunk rewrites s_wave and s_prim)
    }
    uint8_t* sb = reinterpret_cast<uint8_t*>(s_out);
    const uint32_t br = to_byte(r), bg = to_byte(g), bb = to_byte(b);
    if (dwords) {  // W % 4 == 0 and an aligned frame base: every row of every tile starts on a dword
        sb[tid * 3 + 0] = (uint8_t)br;
        sb[tid * 3 + 1] = (uint8_t)bg;
        sb[tid * 3 + 2] = (uint8_t)bb;
        __syncthreads();
        constexpr int kRowDwords = kTile * 3 / 4;  // 12
        const int wpx = min(kTile, W - tx * kTile);
        if (tid < kTile * kRowDwords) {
            const int rr = tid / kRowDwords, c = tid % kRowDwords, ii = ty * kTile + rr;
            if (ii < H && c < wpx * 3 / 4) {
                const int64_t byte0 = (((int64_t)frame * H + ii) * W + (int64_t)tx * kTile) * 3;
                reinterpret_cast<uint32_t*>(out)[byte0 / 4 + c] = s_out[rr * kRowDwords + c];
            }
        }
    } else if (i < H && j < W) {
        uint8_t* o = out + (((int64_t)frame * H + i) * W + j) * 3;
        o[0] = (uint8_t)br;
        o[1] = (uint8_t)bg;
        o[2] = (uint8_t)bb;
    }
}

void render_frames_host(int E, int H, int W, const VmasRenderPrim* prims, int P, const float* verts, uint8_t* out) {
    for (int e = 0; e < E; ++e) {
        const VmasRenderPrim* row = prims + (int64_t)e * P;
        for (int i = 0; i < H; ++i)
            for (int j = 0; j < W; ++j) {
                const float qx = (float)j + 0.5f, qy = (float)(H - i) - 0.5f;
                float r = 1.0f, g = 1.0f, b = 1.0f;
                for (int k = 0; k < P; ++k) {
                    const VmasRenderPrim& pr = row[k];
                    // (the pixel's own 1 x 1 box against the record's: the device culls per tile)
                    if (pr.kind == VMAS_PRIM_NONE || pr.bbox[0] > qx + 0.5f || pr.bbox[2] < qx - 0.5f ||
                        pr.bbox[1] > qy + 0.5f || pr.bbox[3] < qy - 0.5f)
                        continue;
                    composite(pr, verts, qx, qy, r, g, b);
                }
                uint8_t* o = out + (((int64_t)e * H + i) * W + j) * 3;
                o[0] = (uint8_t)to_byte(r);
                o[1] = (uint8_t)to_byte(g);
                o[2] = (uint8_t)to_byte(b);
            }
    }
}

// ------------------------------------------------------------------------------------------------
// the scene: camera and entity layer of a batch
constexpr int kSceneEnts = 16, kSceneLidars = 12, kSceneThreads = 256;
constexpr float kMargin = 2.0f;  // bbox margin in pixels: coverage ends at d = 0.5, a border at |d| = 1.5

struct AgentRef {
    const float* pos;
    int64_t s0;
};

struct SceneArgs {
    VmasRenderEntity ents[kSceneEnts];
    VmasRenderLidar lidars[kSceneLidars];
    AgentRef agents[VMAS_RENDER_MAX_AGENTS];
    VmasRenderScene sc;
    const int64_t* env_index;
    const float* focus_pos;
    VmasRenderPrim* prims;
    float* verts;
    float* bounds;
    int64_t focus_s0;
    float cam_x, cam_y;  // zoom and the viewer's aspect (environment.py:855-858)
    float grid_n;
    int n_agents, n_ents, n_lidars, n_rays, n_static, n_frames;  // n_static > 0: the first launch
};
static_assert(sizeof(SceneArgs) <= 4096, "kernel argument block");

struct Camera {
    float left, right, bottom, top, sx, sy;
};

VR_HD Camera scene_camera(const SceneArgs& a, int64_t env) {
    Camera c;
    if (a.focus_pos) {
        const float px = a.focus_pos[env * a.focus_s0], py = a.focus_pos[env * a.focus_s0 + 1];
        c.left = px - a.cam_x;
        c.right = px + a.cam_x;
        c.bottom = py - a.cam_y;
        c.top = py + a.cam_y;
    } else {
        float mx = 0.0f, my = 0.0f;
        for (int k = 0; k < a.n_agents; ++k) {
            const float* p = a.agents[k].pos + env * a.agents[k].s0;
            mx = fmaxf(mx, fabsf(p[0] - a.sc.origin[0]));
            my = fmaxf(my, fabsf(p[1] - a.sc.origin[1]));
        }
        const float fx = mx + 2.0f * a.sc.max_agent_radius, fy = my + 2.0f * a.sc.max_agent_radius;
        const float vs = fmaxf(fmaxf(fx / a.cam_x, a.sc.zoom), fmaxf(fy / a.cam_y, a.sc.zoom));
        const float cx = a.cam_x * vs, cy = a.cam_y * vs;
        c.left = -cx + a.sc.origin[0];
        c.right = cx + a.sc.origin[0];
        c.bottom = -cy + a.sc.origin[1];
        c.top = cy + a.sc.origin[1];
    }
    c.sx = (float)a.sc.width / (c.right - c.left);
    c.sy = (float)a.sc.height / (c.top - c.bottom);
    return c;
}

VR_HD void prim_clear(VmasRenderPrim& o) {
    o.kind = VMAS_PRIM_NONE;
    o.flags = 0;
    o.rgba[0] = o.rgba[1] = o.rgba[2] = o.rgba[3] = 0.0f;
    o.p[0] = o.p[1] = o.p[2] = o.p[3] = o.p[4] = o.p[5] = 0.0f;
    o.v0 = o.nv = 0;
    o.bbox[0] = o.bbox[1] = o.bbox[2] = o.bbox[3] = 0.0f;
}

VR_HD void prim_seg(VmasRenderPrim& o, float ax, float ay, float bx, float by, float w, float cr, float cg, float cb,
                    float alpha) {
    prim_clear(o);
    o.kind = VMAS_PRIM_SEG;
    o.rgba[0] = cr, o.rgba[1] = cg, o.rgba[2] = cb, o.rgba[3] = alpha;
    o.p[0] = ax, o.p[1] = ay, o.p[2] = bx, o.p[3] = by, o.p[4] = w;
    const float m = 0.5f * line_width(w) + kMargin;
    o.bbox[0] = fminf(ax, bx) - m, o.bbox[1] = fminf(ay, by) - m;
    o.bbox[2] = fmaxf(ax, bx) + m, o.bbox[3] = fmaxf(ay, by) + m;
}

VR_HD void prim_disc(VmasRenderPrim& o, float cx, float cy, float rad, float cr, float cg, float cb, float alpha) {
    prim_clear(o);
    o.kind = VMAS_PRIM_DISC;
    o.flags = VMAS_PRIM_BORDER;
    o.rgba[0] = cr, o.rgba[1] = cg, o.rgba[2] = cb, o.rgba[3] = alpha;
    o.p[0] = cx, o.p[1] = cy, o.p[2] = rad;
    o.bbox[0] = cx - rad - kMargin, o.bbox[1] = cy - rad - kMargin;
    o.bbox[2] = cx + rad + kMargin, o.bbox[3] = cy + rad + kMargin;
}

// item `it` of frame f of this launch: 0 .. n_static-1 the bounds / boundary / grid, then the
// launch's entities, then its LIDAR rays
VR_HD void scene_item(const SceneArgs& a, int f, int it) {
    int64_t env = a.env_index ? a.env_index[f] : (int64_t)f;
    env = env < 0 ? 0 : (env >= a.sc.batch ? a.sc.batch - 1 : env);  // (nothing is read outside the batch)
    const Camera c = scene_camera(a, env);
    VmasRenderPrim* row = a.prims + (int64_t)f * a.sc.n_prims;
    if (it < a.n_static) {
        if (it == 0) {
            float* bo = a.bounds + 4 * (int64_t)f;
            bo[0] = c.left, bo[1] = c.right, bo[2] = c.bottom, bo[3] = c.top;
        } else if (it <= a.sc.n_boundary) {
            const float* s = a.sc.boundary[it - 1];
            prim_seg(row[it - 1], (s[0] - c.left) * c.sx, (s[1] - c.bottom) * c.sy, (s[2] - c.left) * c.sx,
                     (s[3] - c.bottom) * c.sy, 0.7f, 0.25f, 0.25f, 0.25f, 1.0f);
        } else {
            VmasRenderPrim& o = row[a.sc.n_boundary];
            prim_clear(o);
            o.kind = VMAS_PRIM_GRID;
            o.rgba[0] = o.rgba[1] = o.rgba[2] = 0.15f;  // utils.Color.BLACK
            o.rgba[3] = 0.3f;
            // (the line nearest the origin in double: the host lowering of render() does the same)
            const double sxd = (double)a.sc.width / ((double)c.right - (double)c.left);
            const double spd = (double)a.sc.grid_spacing * sxd, halfd = 25.0 * sxd;  // rendering.Grid's length 50
            const double k0 = floor(halfd / spd + 0.5);
            const float half = (float)halfd;
            o.p[0] = (0.0f - c.left) * c.sx, o.p[1] = (0.0f - c.bottom) * c.sy;
            o.p[2] = (float)spd, o.p[3] = half, o.p[4] = 0.5f, o.p[5] = (float)(k0 * spd - halfd);
            o.v0 = (int)-k0, o.nv = (int)((double)a.grid_n - 1.0 - k0);
            o.bbox[0] = o.p[0] - half - kMargin, o.bbox[1] = o.p[1] - half - kMargin;
            o.bbox[2] = o.p[0] + half + kMargin, o.bbox[3] = o.p[1] + half + kMargin;
        }
        return;
    }
    it -= a.n_static;
    if (it < a.n_ents) {
        const VmasRenderEntity& en = a.ents[it];
        VmasRenderPrim& o = row[en.slot];
        const bool shown = !en.mask || en.mask[env];
        const float* col = en.color + env * en.color_s0;
        const float cr = col[0], cg = col[1], cb = col[2];
        const float wx = en.pos[env * en.pos_s0], wy = en.pos[env * en.pos_s0 + 1];
        const float px = (wx - c.left) * c.sx, py = (wy - c.bottom) * c.sy;
        if (en.flags & VMAS_RENDER_ACTION) {
            VmasRenderPrim& oa = row[en.action_slot];
            if (shown) {
                const float* fo = en.force + env * en.force_s0;
                const float ex = wx + fo[0] * en.action_scale, ey = wy + fo[1] * en.action_scale;
                prim_seg(oa, px, py, (ex - c.left) * c.sx, (ey - c.bottom) * c.sy, 2.0f, cr, cg, cb, 1.0f);
            } else {
                prim_clear(oa);
            }
        }
        if (!shown) {
            prim_clear(o);
            return;
        }
        const float rot = en.rot[env * en.rot_s0], cs = cosf(rot), sn = sinf(rot);
        if (en.shape == VMAS_SPHERE) {
            prim_disc(o, px, py, en.radius * c.sx, cr, cg, cb, en.alpha);
        } else if (en.shape == VMAS_LINE) {
            const float hx = 0.5f * en.length * cs, hy = 0.5f * en.length * sn;
            prim_seg(o, (wx - hx - c.left) * c.sx, (wy - hy - c.bottom) * c.sy, (wx + hx - c.left) * c.sx,
                     (wy + hy - c.bottom) * c.sy, en.width, cr, cg, cb, en.alpha);
        } else {
            prim_clear(o);
            o.kind = VMAS_PRIM_POLY;
            o.flags = VMAS_PRIM_BORDER;
            o.rgba[0] = cr, o.rgba[1] = cg, o.rgba[2] = cb, o.rgba[3] = en.alpha;
            o.v0 = (f * a.sc.n_boxes + en.vert_slot) * 4;
            o.nv = 4;
            float* v = a.verts + 2 * (int64_t)o.v0;
            const float hl = 0.5f * en.length, hw = 0.5f * en.width;
            float xmin = kFar, ymin = kFar, xmax = -kFar, ymax = -kFar;
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // (l, b), (l, t), (r, t), (r, b)
                const float lx = (k < 2) ? -hl : hl, ly = (k == 1 || k == 2) ? hw : -hw;
                const float vx = (wx + (lx * cs - ly * sn) - c.left) * c.sx;
                const float vy = (wy + (lx * sn + ly * cs) - c.bottom) * c.sy;
                v[2 * k] = vx, v[2 * k + 1] = vy;
                xmin = fminf(xmin, vx), xmax = fmaxf(xmax, vx);
                ymin = fminf(ymin, vy), ymax = fmaxf(ymax, vy);
            }
            o.bbox[0] = xmin - kMargin, o.bbox[1] = ymin - kMargin, o.bbox[2] = xmax + kMargin, o.bbox[3] = ymax + kMargin;
        }
        return;
    }
    it -= a.n_ents;
    int l = 0;
    while (l < a.n_lidars - 1 && it >= a.lidars[l].n_rays) {
        it -= a.lidars[l].n_rays;
        ++l;
    }
    const VmasRenderLidar& li = a.lidars[l];
    VmasRenderPrim& oseg = row[li.slot + 2 * it];
    VmasRenderPrim& odisc = row[li.slot + 2 * it + 1];
    if (li.mask && !li.mask[env]) {
        prim_clear(oseg);
        prim_clear(odisc);
        return;
    }
    const float wx = li.pos[env * li.pos_s0], wy = li.pos[env * li.pos_s0 + 1];
    const float ang = li.angles[env * li.angles_s0 + it] + li.rot[env * li.rot_s0];
    const float dist = li.dist[env * li.dist_s0 + it];
    const float ex = wx + cosf(ang) * dist, ey = wy + sinf(ang) * dist;
    const float qx = (ex - c.left) * c.sx, qy = (ey - c.bottom) * c.sy;
    prim_seg(oseg, (wx - c.left) * c.sx, (wy - c.bottom) * c.sy, qx, qy, 0.05f, 0.0f, 0.0f, 0.0f, li.alpha);
    prim_disc(odisc, qx, qy, 0.01f * c.sx, li.rgb[0], li.rgb[1], li.rgb[2], li.alpha);
}

__global__ void __launch_bounds__(kSceneThreads) k_render_scene(SceneArgs a) {
    const int items = a.n_static + a.n_ents + a.n_rays;
    const int64_t gid = (int64_t)blockIdx.x * kSceneThreads + threadIdx.x;
    if (gid >= (int64_t)a.n_frames * items) return;
    scene_item(a, (int)(gid / items), (int)(gid % items));
}

}  // namespace

extern "C" int32_t vmas_render_frames(int32_t device, int32_t n_frames, int32_t height, int32_t width,
                                      const VmasRenderPrim* prims, int32_t n_prims, const float* verts, int32_t n_verts,
                                      uint8_t* out, void* stream) {
    if (n_frames < 0 || height <= 0 || width <= 0 || height > 16384 || width > 16384 || n_prims < 0 || n_verts < 0 ||
        !out || (n_prims > 0 && !prims) || (n_verts > 0 && !verts))
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_render_frames: bad arguments");
    if (n_frames == 0) return VMAS_OK;
    const int tiles_x = (width + kTile - 1) / kTile, tiles_y = (height + kTile - 1) / kTile;
    const int64_t blocks = (int64_t)n_frames * tiles_x * tiles_y;
    if (blocks > 0x7fffffffLL || (int64_t)n_frames * n_prims > 0x7fffffffLL)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_render_frames: %d frames of %d x %d are too many for one call", n_frames,
                              height, width);
    if (device < 0) {
        // (a POLY's vertex range is checked where the table can be read: on the host)
        for (int64_t k = 0; k < (int64_t)n_frames * n_prims; ++k) {
            const VmasRenderPrim& pr = prims[k];
            if (pr.kind < VMAS_PRIM_NONE || pr.kind > VMAS_PRIM_GRID)
                return vmas_aux::fail(VMAS_E_INVALID, "vmas_render_frames: record %lld has kind %d", (long long)k, pr.kind);
            if (pr.kind == VMAS_PRIM_POLY && (pr.nv < 3 || pr.v0 < 0 || (int64_t)pr.v0 + pr.nv > n_verts))
                return vmas_aux::fail(VMAS_E_INVALID, "vmas_render_frames: record %lld indexes vertices %d..%d of %d",
                                      (long long)k, pr.v0, pr.v0 + pr.nv, n_verts);
        }
        render_frames_host(n_frames, height, width, prims, n_prims, verts, out);
        return VMAS_OK;
    }
    VMAS_AUX_HIP(hipSetDevice(device));
    const int dwords = (width % 4 == 0) && (((uintptr_t)out & 3) == 0);
    hipLaunchKernelGGL(k_render_frames, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, prims, n_prims,
                       verts, n_verts, out, height, width, tiles_x, tiles_x * tiles_y, dwords);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

extern "C" int32_t vmas_render_scene(int32_t device, int32_t n_frames, const int64_t* env_index,
                                     const VmasRenderEntity* entities, int32_t n_entities, const VmasRenderLidar* lidars,
                                     int32_t n_lidars, const VmasRenderScene* scene, VmasRenderPrim* prims, float* verts,
                                     float* bounds, void* stream) {
    if (n_frames < 0 || n_entities <= 0 || !entities || n_lidars < 0 || (n_lidars > 0 && !lidars) || !scene || !prims ||
        !bounds)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_render_scene: bad arguments");
    const VmasRenderScene& sc = *scene;
    if (sc.batch <= 0 || (!env_index && n_frames > sc.batch) || sc.width <= 0 || sc.height <= 0 || !(sc.zoom > 0.0f) || sc.n_boundary < 0 || sc.n_boundary > 4 || sc.n_boxes < 0 ||
        (sc.n_boxes > 0 && !verts) || sc.focus >= n_entities || (sc.plot_grid && !(sc.grid_spacing > 0.0f)))
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_render_scene: bad scene");
    const int n_fixed = sc.n_boundary + (sc.plot_grid ? 1 : 0);
    if (sc.n_prims < n_fixed || (int64_t)n_frames * sc.n_prims > 0x7fffffffLL ||
        (int64_t)n_frames * std::max(sc.n_boxes, 1) * 4 > 0x7fffffffLL)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_render_scene: bad table size");
    SceneArgs base;
    memset(&base, 0, sizeof(base));
    base.sc = sc;
    for (int i = 0; i < n_entities; ++i) {
        const VmasRenderEntity& en = entities[i];
        const bool act = en.flags & VMAS_RENDER_ACTION;
        if (!en.pos || !en.rot || !en.color || en.shape < VMAS_SPHERE || en.shape > VMAS_LINE || en.slot < n_fixed ||
            en.slot >= sc.n_prims || (act && (!en.force || en.action_slot < n_fixed || en.action_slot >= sc.n_prims)) ||
            (en.shape == VMAS_BOX && (en.vert_slot < 0 || en.vert_slot >= sc.n_boxes)))
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_render_scene: bad entity %d", i);
        if (en.flags & VMAS_RENDER_AGENT) {
            if (base.n_agents == VMAS_RENDER_MAX_AGENTS)
                return vmas_aux::fail(VMAS_E_UNSUPPORTED, "vmas_render_scene: more than %d agents", VMAS_RENDER_MAX_AGENTS);
            base.agents[base.n_agents].pos = en.pos;
            base.agents[base.n_agents].s0 = en.pos_s0;
            ++base.n_agents;
        }
    }
    for (int i = 0; i < n_lidars; ++i) {
        const VmasRenderLidar& li = lidars[i];
        if (!li.pos || !li.rot || !li.angles || !li.dist || li.n_rays <= 0 || li.slot < n_fixed ||
            (int64_t)li.slot + 2 * (int64_t)li.n_rays > sc.n_prims)
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_render_scene: bad lidar %d", i);
    }
    if (sc.focus < 0 && base.n_agents == 0)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_render_scene: the shared camera needs an agent");
    if (n_frames == 0) return VMAS_OK;
    if (sc.focus >= 0) {
        base.focus_pos = entities[sc.focus].pos;
        base.focus_s0 = entities[sc.focus].pos_s0;
    }
    const double aspect = (double)sc.width / (double)sc.height;
    base.cam_x = aspect < 1.0 ? sc.zoom : (float)((double)sc.zoom * aspect);
    base.cam_y = aspect < 1.0 ? (float)((double)sc.zoom / aspect) : sc.zoom;
    base.grid_n = sc.plot_grid ? (float)std::ceil(50.0 / (double)sc.grid_spacing) : 0.0f;
    base.env_index = env_index;
    base.prims = prims;
    base.verts = verts;
    base.bounds = bounds;
    base.n_frames = n_frames;
    if (device >= 0) VMAS_AUX_HIP(hipSetDevice(device));
    const int launches = std::max((n_entities + kSceneEnts - 1) / kSceneEnts, (n_lidars + kSceneLidars - 1) / kSceneLidars);
    for (int c = 0; c < launches; ++c) {
        SceneArgs a = base;
        a.n_static = c == 0 ? 1 + n_fixed : 0;
        a.n_ents = std::max(0, std::min(kSceneEnts, n_entities - c * kSceneEnts));
        a.n_lidars = std::max(0, std::min(kSceneLidars, n_lidars - c * kSceneLidars));
        for (int i = 0; i < a.n_ents; ++i) a.ents[i] = entities[c * kSceneEnts + i];
        a.n_rays = 0;
        for (int i = 0; i < a.n_lidars; ++i) {
            a.lidars[i] = lidars[c * kSceneLidars + i];
            a.n_rays += a.lidars[i].n_rays;
        }
        const int items = a.n_static + a.n_ents + a.n_rays;
        const int64_t total = (int64_t)n_frames * items;
        if (device < 0) {
            for (int f = 0; f < n_frames; ++f)
                for (int it = 0; it < items; ++it) scene_item(a, f, it);
            continue;
        }
        const int64_t blocks = (total + kSceneThreads - 1) / kSceneThreads;
        if (blocks > 0x7fffffffLL) return vmas_aux::fail(VMAS_E_INVALID, "vmas_render_scene: too many frames for one call");
        hipLaunchKernelGGL(k_render_scene, dim3((unsigned)blocks), dim3(kSceneThreads), 0, (hipStream_t)stream, a);
        VMAS_AUX_HIP(hipGetLastError());
    }
    return VMAS_OK;
}
