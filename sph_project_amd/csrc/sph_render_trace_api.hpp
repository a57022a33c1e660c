// sph_render_trace_api.hpp -- the traced mesh frames of the SphRender object: the mode's parameters, its buffers, the frame
// itself (called by sph_render_mesh_end while the mode is on), statistics and the downloads of the hierarchy and of the recorded paths.
// Host code, included behind sph_render_api.hpp by sph_api.hip; the kernels are in sph_render_trace.hpp.
#pragma once

enum TraceBufId { TRB_CORNER, TRB_ST, TRB_KEY0, TRB_KEY1, TRB_HIST, TRB_LEFT, TRB_RIGHT, TRB_PARENT, TRB_SKIP, TRB_ARRIVE, TRB_BOX, TRB_SMALL, TRB_REC, TRB_COUNT_ };
#define TRACE_MAX_TRIANGLES (((int64_t)1 << 30) - 1)   // node ids are ints: 2 n - 1 nodes

struct RendTrace {
    SphRenderTraceParams prm{};
    DevBuf buf[TRB_COUNT_];
    hipEvent_t ev[7] = {};
    SphRenderTraceStats stats{};
    bool have_frame = false;     // the frame held is a traced one: stats, the hierarchy and (record) the paths belong to it
    bool have_paths = false;
    int64_t n = 0, nt = 0;       // kept triangles and triangles of that frame
};

static void rend_trace_free(SphRender *r) {
    RendTrace *t = r->tr;
    if (!t) return;
    hipSetDevice(r->device);
    if (r->stream) hipStreamSynchronize(r->stream);
    for (DevBuf &b : t->buf) b.release();
    for (hipEvent_t e : t->ev) if (e) hipEventDestroy(e);
    delete t;
    r->tr = nullptr;
}

extern "C" int sph_render_set_trace(SphRender *r, const SphRenderTraceParams *params) {
    if (!r) return SPH_ERR_INVALID;
    if (!params) { rend_trace_free(r); return SPH_OK; }
    const SphRenderTraceParams p = *params;
    if (p.max_depth < 1 || p.max_depth > 64) return fail(r, SPH_ERR_INVALID, "sph_render_set_trace: max_depth %d outside 1..64", p.max_depth);
    if (!(p.ior >= 1.0f) || !std::isfinite(p.ior)) return fail(r, SPH_ERR_INVALID, "sph_render_set_trace: ior %g must be finite and at least 1", (double)p.ior);
    if (!(p.absorb >= 0.0f) || !std::isfinite(p.absorb)) return fail(r, SPH_ERR_INVALID, "sph_render_set_trace: absorb %g must be finite and not negative", (double)p.absorb);
    if (!(p.floor_cell > 0.0f) || !std::isfinite(p.floor_cell)) return fail(r, SPH_ERR_INVALID, "sph_render_set_trace: floor_cell %g must be finite and positive", (double)p.floor_cell);
    if ((p.shadows | p.floor | p.use_bvh | p.record) & ~1) return fail(r, SPH_ERR_INVALID, "sph_render_set_trace: shadows, floor, use_bvh and record are 0 or 1");
    if (r->frame == RF_ON_RANK0 || r->cstats.ranks > 1)
        return fail(r, SPH_ERR_UNSUPPORTED, "sph_render_set_trace: the renderer composites the layers of a sharded handle (traced frames are not composited)");
    if (r->mesh_open) return fail(r, SPH_ERR_INVALID, "sph_render_set_trace: between sph_render_mesh_begin and sph_render_mesh_end");
    if (!r->tr) {
        HIPCHK(r, hipSetDevice(r->device));
        r->tr = new RendTrace();
        for (hipEvent_t &e : r->tr->ev)
            if (hipEventCreate(&e) != hipSuccess) { rend_trace_free(r); return fail(r, SPH_ERR_HIP, "sph_render_set_trace: event"); }
    }
    r->tr->prm = p;
    r->tr->have_frame = r->tr->have_paths = false;   // (what is held was traced with other parameters)
    return SPH_OK;
}

extern "C" int sph_render_mesh_material(SphRender *r, int material, int flip) {
    if (!r) return SPH_ERR_INVALID;
    if (!r->mesh_open || r->mesh_rec.empty())
        return fail(r, SPH_ERR_INVALID, "sph_render_mesh_material: no mesh added since sph_render_mesh_begin");
    if ((material != SPH_RENDER_MATERIAL_DIFFUSE && material != SPH_RENDER_MATERIAL_WATER) || (flip & ~1))
        return fail(r, SPH_ERR_INVALID, "sph_render_mesh_material: material %d (0 diffuse, 1 water), flip %d (0 or 1)", material, flip);
    r->mesh_rec.back().mat = material | (flip << 1);
    return SPH_OK;
}

// the frame of sph_render_mesh_end while the mode is on: m is set, the mesh table is on its way to the device, stage mark 0 is the caller's
static int rend_trace_end(SphRender *r, MeshDev &m) {
    RendTrace *tr = r->tr;
    RenderDev &d = r->d;
    tr->have_frame = tr->have_paths = false;
    tr->stats = SphRenderTraceStats{};
    if (m.nt > TRACE_MAX_TRIANGLES)
        return fail(r, SPH_ERR_UNSUPPORTED, "sph_render_mesh_end: %lld triangles, a traced frame holds at most %lld", (long long)m.nt, (long long)TRACE_MAX_TRIANGLES);
    const SphRenderTraceParams &p = tr->prm;
    const size_t nt = (size_t)std::max<int64_t>(m.nt, 1), px = (size_t)d.W * d.H;
    const size_t tiles = (nt + TRACE_SORT_TILE - 1) / TRACE_SORT_TILE;
    const size_t rec_bytes = p.record ? px * (size_t)p.max_depth * TRACE_REC_WORDS * 4 : 0;
    DevBuf *b = tr->buf;
    int rc = b[TRB_CORNER].reserve(r, nt * 3 * sizeof(float4));
    if (!rc) rc = b[TRB_ST].reserve(r, nt * 4);
    if (!rc) rc = b[TRB_KEY0].reserve(r, nt * 8);
    if (!rc) rc = b[TRB_KEY1].reserve(r, nt * 8);
    if (!rc) rc = b[TRB_HIST].reserve(r, (tiles + 1) * 256 * 4);
    if (!rc) rc = b[TRB_LEFT].reserve(r, nt * 4);
    if (!rc) rc = b[TRB_RIGHT].reserve(r, nt * 4);
    if (!rc) rc = b[TRB_PARENT].reserve(r, 2 * nt * 4);
    if (!rc) rc = b[TRB_SKIP].reserve(r, 2 * nt * 4);
    if (!rc) rc = b[TRB_ARRIVE].reserve(r, nt * 4);
    if (!rc) rc = b[TRB_BOX].reserve(r, 2 * nt * 6 * 4);
    if (!rc) rc = b[TRB_SMALL].reserve(r, 32 + TC_COUNT_ * 8);
    if (!rc && rec_bytes) rc = b[TRB_REC].reserve(r, rec_bytes);
    if (rc) return rc;
    TraceDev t{};
    t.corner = (float4 *)b[TRB_CORNER].p; t.st = (int *)b[TRB_ST].p;
    t.key[0] = (unsigned long long *)b[TRB_KEY0].p; t.key[1] = (unsigned long long *)b[TRB_KEY1].p;
    t.hist = (unsigned *)b[TRB_HIST].p;
    t.left = (int *)b[TRB_LEFT].p; t.right = (int *)b[TRB_RIGHT].p; t.parent = (int *)b[TRB_PARENT].p; t.skip = (int *)b[TRB_SKIP].p;
    t.arrive = (int *)b[TRB_ARRIVE].p; t.box = (float *)b[TRB_BOX].p;
    t.bnd = (unsigned *)b[TRB_SMALL].p; t.ctr = (unsigned long long *)((char *)b[TRB_SMALL].p + 32);
    t.rec = rec_bytes ? (float *)b[TRB_REC].p : nullptr;
    const SphRenderParams &rp = r->prm;
    for (int k = 0; k < 3; ++k) t.light[k] = (float)rp.light_pos[k];
    t.floor = (p.floor && rp.draw_box) ? 1 : 0;
    t.floor_y = (float)rp.box_lo[1];
    t.floor_lo[0] = (float)rp.box_lo[0]; t.floor_lo[1] = (float)rp.box_lo[2];
    t.floor_hi[0] = (float)rp.box_hi[0]; t.floor_hi[1] = (float)rp.box_hi[2];
    t.cell = (float)((double)p.floor_cell * rp.radius);
    t.ior = p.ior; t.absorb = (float)((double)p.absorb / rp.radius);
    t.max_depth = p.max_depth; t.shadows = p.shadows; t.use_bvh = p.use_bvh;
    hipStream_t s = r->stream;
    HIPCHK(r, hipMemsetAsync(d.cnt, 0, 64, s));
    HIPCHK(r, hipMemsetAsync(t.bnd, 0xff, 12, s));
    HIPCHK(r, hipMemsetAsync(t.bnd + 3, 0, 20, s));
    HIPCHK(r, hipMemsetAsync(t.ctr, 0, TC_COUNT_ * 8, s));
    HIPCHK(r, hipMemsetAsync(t.arrive, 0, nt * 4, s));
    if (rec_bytes) HIPCHK(r, hipMemsetAsync(t.rec, 0, rec_bytes, s));
    HIPCHK(r, hipEventRecord(tr->ev[0], s));
    r->L->render_trace_setup(m, t, s);
    HIPCHK(r, hipEventRecord(tr->ev[1], s));
    r->L->render_trace_sort(m, t, s);
    HIPCHK(r, hipEventRecord(tr->ev[2], s));
    r->L->render_trace_hierarchy(m, t, s);
    HIPCHK(r, hipEventRecord(tr->ev[3], s));
    r->L->render_trace_fit(m, t, s);
    HIPCHK(r, hipEventRecord(tr->ev[4], s));
    r->L->render_trace_shade(d, m, t);
    HIPCHK(r, hipEventRecord(tr->ev[5], s));
    r->L->render_trace_finish(d);
    HIPCHK(r, hipEventRecord(tr->ev[6], s));
    unsigned long long c[8], tc[TC_COUNT_];
    HIPCHK(r, hipMemcpyAsync(tc, t.ctr, sizeof(tc), hipMemcpyDeviceToHost, s));
    { int rc2 = rend_close(r, c, RF_MESH); if (rc2) return rc2; }
    SphRenderTraceStats &o = tr->stats;
    o.triangles = (int64_t)tc[TC_KEPT]; o.nodes = o.triangles ? 2 * o.triangles - 1 : 0; o.depth = (int64_t)tc[TC_DEPTH];
    o.skipped_nonfinite = (int64_t)tc[TC_NONFINITE]; o.skipped_degenerate = (int64_t)tc[TC_DEGENERATE]; o.bad_index = (int64_t)tc[TC_BAD_INDEX];
    o.rays_primary = (int64_t)tc[TC_RAYS_PRIMARY]; o.rays_path = (int64_t)tc[TC_RAYS_PATH]; o.rays_reflect = (int64_t)tc[TC_RAYS_REFLECT];
    o.rays_shadow = (int64_t)tc[TC_RAYS_SHADOW]; o.node_visits = (int64_t)tc[TC_VISITS]; o.triangle_tests = (int64_t)tc[TC_TESTS];
    o.truncated = (int64_t)tc[TC_TRUNCATED]; o.aborted_rays = (int64_t)tc[TC_ABORTED];
    o.ms_setup = ev_ms(tr->ev[0], tr->ev[1]); o.ms_sort = ev_ms(tr->ev[1], tr->ev[2]); o.ms_hierarchy = ev_ms(tr->ev[2], tr->ev[3]);
    o.ms_fit = ev_ms(tr->ev[3], tr->ev[4]); o.ms_trace = ev_ms(tr->ev[4], tr->ev[5]); o.ms_finish = ev_ms(tr->ev[5], tr->ev[6]);
    o.ms_total = ev_ms(tr->ev[0], tr->ev[6]);
    tr->n = o.triangles; tr->nt = m.nt;
    tr->have_frame = true; tr->have_paths = rec_bytes != 0;
    SphRenderMeshStats &ms = r->mstats;
    ms.meshes = (int64_t)m.nm; ms.triangles = r->mesh_nt; ms.vertices = r->mesh_nv;
    ms.skipped_nonfinite = o.skipped_nonfinite; ms.skipped_degenerate = o.skipped_degenerate; ms.bad_index = o.bad_index;
    ms.covered_pixels = (int64_t)c[4];
    ms.ms_total = r->clk[1].ms(0, 1) + o.ms_total;
    if (o.bad_index)
        return fail(r, SPH_ERR_INVALID, "sph_render_mesh_end: %lld triangle(s) with a vertex index outside their mesh (skipped; the frame holds the rest)",
                    (long long)o.bad_index);
    return SPH_OK;
}

static int rend_trace_held(SphRender *r, const char *who) {
    if (!r->tr) return fail(r, SPH_ERR_INVALID, "%s: the trace mode is off (sph_render_set_trace)", who);
    if (r->frame != RF_MESH || !r->tr->have_frame) return fail(r, SPH_ERR_INVALID, "%s: the frame held is not a traced mesh frame", who);
    return SPH_OK;
}

extern "C" int sph_render_trace_stats(SphRender *r, SphRenderTraceStats *out) {
    if (!r || !out) return SPH_ERR_INVALID;
    { int rc = rend_trace_held(r, "sph_render_trace_stats"); if (rc) return rc; }
    *out = r->tr->stats;
    return SPH_OK;
}

extern "C" int sph_render_trace_download_bvh(SphRender *r, int32_t *left, int32_t *right, float *boxes, int32_t *leaf_triangle) {
    if (!r) return SPH_ERR_INVALID;
    { int rc = rend_trace_held(r, "sph_render_trace_download_bvh"); if (rc) return rc; }
    RendTrace *t = r->tr;
    const size_t n = (size_t)t->n;
    if (n == 0) return SPH_OK;
    HIPCHK(r, hipSetDevice(r->device));
    if (left && n > 1) HIPCHK(r, hipMemcpy(left, t->buf[TRB_LEFT].p, (n - 1) * 4, hipMemcpyDeviceToHost));
    if (right && n > 1) HIPCHK(r, hipMemcpy(right, t->buf[TRB_RIGHT].p, (n - 1) * 4, hipMemcpyDeviceToHost));
    if (boxes) HIPCHK(r, hipMemcpy(boxes, t->buf[TRB_BOX].p, (2 * n - 1) * 24, hipMemcpyDeviceToHost));
    if (leaf_triangle) {
        std::vector<uint64_t> key(n);
        HIPCHK(r, hipMemcpy(key.data(), t->buf[TRB_KEY0].p, n * 8, hipMemcpyDeviceToHost));
        for (size_t j = 0; j < n; ++j) leaf_triangle[j] = (int32_t)(uint32_t)key[j];
    }
    return SPH_OK;
}

extern "C" int sph_render_trace_download_paths(SphRender *r, float *segments) {
    if (!r || !segments) return SPH_ERR_INVALID;
    { int rc = rend_trace_held(r, "sph_render_trace_download_paths"); if (rc) return rc; }
    RendTrace *t = r->tr;
    if (!t->have_paths) return fail(r, SPH_ERR_INVALID, "sph_render_trace_download_paths: the frame held was traced without record = 1");
    HIPCHK(r, hipSetDevice(r->device));
    const size_t bytes = (size_t)r->d.W * r->d.H * (size_t)t->prm.max_depth * SPH_RENDER_TRACE_SEGMENT_WORDS * 4;
    HIPCHK(r, hipMemcpy(segments, t->buf[TRB_REC].p, bytes, hipMemcpyDeviceToHost));
    return SPH_OK;
}
