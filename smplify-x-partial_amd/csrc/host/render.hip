// render.hip -- sfx_render_meshes (include/sfx.h): the stateless entry of the mesh rasteriser.  Checks the arguments, clears the
// visibility buffer and the drop counters and enqueues the four kernels of csrc/raster.hip on the caller's stream, each under
// its own profiler name (render_project, render_vnormals, render_clear, render_cover, render_resolve: tools/bench_render.py).
// No handle, no allocation, no synchronisation.
#include "host.h"

#define RS_MAX_ELEMS (1 << 28)      // vertices or faces of one mesh: 3 * F and every vertex offset stay inside int32

extern "C" int sfx_render_meshes(const sfx_render_cfg* cfg, int32_t B, int32_t V, int32_t F, int32_t H, int32_t W,
                                 const float* verts_dev, const int32_t* faces_dev, const int32_t* vf_offsets_dev,
                                 const int32_t* vf_faces_dev, const float* cam_rot_dev, const float* cam_t_dev,
                                 const float* focal_dev, const float* center_dev, const unsigned char* background_dev,
                                 unsigned long long* vis_scratch_dev, float* vnormal_scratch_dev, int32_t* snapped_scratch_dev,
                                 unsigned char* rgba_dev, float* depth_dev, int32_t* tri_dev, float* screen_dev,
                                 int32_t* dropped_dev, void* stream) {
    if (B == 0) return 0;
    if (B < 0) { sfx_set_error("sfx_render_meshes: B = %d", B); return -1; }
    if (!cfg) { sfx_set_error("sfx_render_meshes: cfg is NULL"); return -1; }
    if (cfg->n_lights < 0 || cfg->n_lights > SFX_RENDER_MAX_LIGHTS) {
        sfx_set_error("sfx_render_meshes: %d lights, supported 0..%d", cfg->n_lights, SFX_RENDER_MAX_LIGHTS); return -1; }
    if (!(cfg->znear > 0.f)) { sfx_set_error("sfx_render_meshes: znear = %g, must be > 0", (double)cfg->znear); return -1; }
    if (V < 1 || F < 1 || V > RS_MAX_ELEMS || F > RS_MAX_ELEMS) {
        sfx_set_error("sfx_render_meshes: V = %d vertices, F = %d faces, supported 1..%d", V, F, RS_MAX_ELEMS); return -1; }
    if (H < 1 || W < 1 || (long long)H * W > INT32_MAX || (long long)H * W * B > INT32_MAX) {
        sfx_set_error("sfx_render_meshes: %d images of %d x %d: H, W >= 1 and B * H * W within int32 are needed", B, H, W); return -1; }
    if (!verts_dev || !faces_dev || !vf_offsets_dev || !vf_faces_dev || !cam_t_dev || !focal_dev || !center_dev ||
        !vis_scratch_dev || !vnormal_scratch_dev || !snapped_scratch_dev) {
        sfx_set_error("sfx_render_meshes: a required pointer is NULL"); return -1; }
    RasterArgs A{};
    A.B = B; A.V = V; A.F = F; A.H = H; A.W = W; A.n_lights = cfg->n_lights; A.znear = cfg->znear;
    for (int c = 0; c < 3; ++c) A.base[c] = cfg->base_rgb[c];
    for (int l = 0; l < cfg->n_lights; ++l) {
        for (int c = 0; c < 3; ++c) A.light_dir[l][c] = cfg->light_dir[l][c];
        A.light_int[l] = cfg->light_intensity[l];
    }
    A.verts = verts_dev; A.faces = faces_dev; A.vf_off = vf_offsets_dev; A.vf_faces = vf_faces_dev;
    A.rot = cam_rot_dev; A.trans = cam_t_dev; A.focal = focal_dev; A.center = center_dev; A.background = background_dev;
    A.vis = vis_scratch_dev; A.vnormal = vnormal_scratch_dev; A.snapped = snapped_scratch_dev;
    A.rgba = rgba_dev; A.depth = depth_dev; A.tri = tri_dev; A.screen = screen_dev; A.dropped = dropped_dev;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope p("render_clear", s, B);
        SFX_CHECK(hipMemsetAsync(vis_scratch_dev, 0xff, sizeof(unsigned long long) * (size_t)B * H * W, s));
        if (dropped_dev) SFX_CHECK(hipMemsetAsync(dropped_dev, 0, sizeof(int32_t) * (size_t)B, s));
    }
    static const char* const names[RS_STAGES] = {"render_project", "render_vnormals", "render_cover", "render_resolve"};
    const bool shade = rgba_dev != nullptr;                 // the normals are read by the colour alone
    for (int stage = 0; stage < RS_STAGES; ++stage) {
        if (stage == RS_STAGE_VNORMALS && !shade) continue;
        if (stage == RS_STAGE_RESOLVE && !rgba_dev && !depth_dev && !tri_dev) continue;
        ProfScope p(names[stage], s, B);
        for (int b0 = 0; b0 < B; b0 += RS_GRID_Y) launch_raster_stage(A, stage, b0, std::min(B - b0, RS_GRID_Y), s);
        SFX_CHECK(hipGetLastError());
    }
    return 0;
}
