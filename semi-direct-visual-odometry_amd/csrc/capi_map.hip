// capi_map.hip — C ABI: map reprojection planning and trajectory output (host code only).
#include <algorithm>
#include <cmath>

#include "capi_ctx.h"
#include "svo_math.h"

using namespace svo::shim;

extern "C" {
// ------------------------------------------------------------------ map reprojection (host planning)
// Frame::world2image (src/frame.cpp:83-92) with PinholeCamera::project2d (src/pinhole_camera.cpp:53-57):
// the same arithmetic, in the same order, as the device and oracle paths (no FMA contraction).
static inline void world2image(const svo_camera* cam, const svo::SE3& T, const double* p, double* px) {
    const svo::V3 c = svo::se3_act(T, svo::V3{p[0], p[1], p[2]});
    px[0] = cam->fx * (c.x / c.z) + cam->cx;
    px[1] = cam->fy * (c.y / c.z) + cam->cy;
}
static inline bool in_frame(const svo_camera* cam, const double* px, double b) {  // src/pinhole_camera.cpp:163-168
    return px[0] >= b && px[1] >= b && px[0] < cam->width - b && px[1] < cam->height - b;
}

int svo_world2image(const svo_camera* cam, const double* pose, int32_t n, const double* points, double* px) {
    if (!cam || !pose || n < 0 || (n > 0 && (!points || !px))) return fail(SVO_ERR_ARG, "null argument");
    const svo::SE3 T = svo::se3_load(pose);
    for (int32_t i = 0; i < n; ++i) world2image(cam, T, points + 3 * i, px + 2 * i);
    return SVO_OK;
}

int svo_map_reproject_plan(const svo_camera* cam, int32_t cell_size, int32_t n_cells, const int32_t* cell_order,
                           const double* cur_pose, uint64_t cur_id, int32_t n_kf, const int32_t* kf_feat_off,
                           const int32_t* feat_point, int32_t n_points, const double* point_pos,
                           const uint32_t* point_type, uint64_t* point_last, int32_t* overlap, int32_t* n_sel,
                           int32_t* sel_feat, int32_t* sel_cell, double* sel_px, int32_t* matches, int32_t* trials) {
    if (!cam || !cell_order || !cur_pose || !kf_feat_off || !overlap || !n_sel || !sel_feat || !sel_cell || !sel_px ||
        !matches || !trials || (n_points > 0 && (!point_pos || !point_type || !point_last)))
        return fail(SVO_ERR_ARG, "null argument");
    if (cell_size < 1) return fail(SVO_ERR_ARG, "cell_size %d", cell_size);
    const int32_t cols = (int32_t)std::ceil((double)cam->width / cell_size);  // src/map.cpp:226-227
    const int32_t rows = (int32_t)std::ceil((double)cam->height / cell_size);
    if (n_cells != cols * rows) return fail(SVO_ERR_ARG, "n_cells %d != %d x %d", n_cells, cols, rows);
    if (n_kf < 0 || (kf_feat_off[n_kf] > 0 && !feat_point)) return fail(SVO_ERR_ARG, "bad feature table");
    for (int32_t i = 0; i < n_cells; ++i)
        if (cell_order[i] < 0 || cell_order[i] >= n_cells) return fail(SVO_ERR_ARG, "cell_order[%d] out of range", i);
    const svo::SE3 T = svo::se3_load(cur_pose);
    std::vector<std::vector<int32_t>> cells(n_cells);  // resetGrid (:250-258)
    double px[2];
    for (int32_t k = 0; k < n_kf; ++k) {  // closeKeyframes: ref, then ref->lastKeyframe (:441-461)
        overlap[k] = 0;
        for (int32_t f = kf_feat_off[k]; f < kf_feat_off[k + 1]; ++f) {
            const int32_t p = feat_point[f];
            if (p < 0) continue;
            if (p >= n_points) return fail(SVO_ERR_ARG, "feature %d: point %d out of range", f, p);
            if (point_last[p] == cur_id) continue;
            point_last[p] = cur_id;
            world2image(cam, T, point_pos + 3 * p, px);  // reprojectPoint (:481-492)
            if (!in_frame(cam, px, 3.0)) continue;
            const uint32_t cell = (uint32_t)(int32_t)px[1] / (uint32_t)cell_size * (uint32_t)cols +
                                  (uint32_t)(int32_t)px[0] / (uint32_t)cell_size;
            cells[cell].push_back(f);
            ++overlap[k];
        }
    }
    int32_t m = 0, t = 0, ns = 0;
    for (int32_t i = 0; i < n_cells; ++i) {  // (:463-477)
        const int32_t idx = cell_order[i];
        std::vector<int32_t>& c = cells[idx];
        if (!c.empty()) {
            // reprojectCell (:505-570): std::sort by point type, descending (the reference's own
            // comparator, so cells past 16 candidates keep libstdc++'s order), first non-deleted wins;
            // its FeatureAlignment result is not used to accept or reject
            std::sort(c.begin(), c.end(), [&](int32_t a, int32_t b) { return point_type[feat_point[a]] > point_type[feat_point[b]]; });
            for (int32_t f : c) {
                ++t;
                if (point_type[feat_point[f]] == 1u) continue;  // Point::PointType::DELETED
                sel_feat[ns] = f;
                sel_cell[ns] = idx;
                world2image(cam, T, point_pos + 3 * feat_point[f], sel_px + 2 * ns);
                ++ns;
                ++m;
                break;
            }
        }
        if (m > 150) break;
    }
    *n_sel = ns;
    *matches = m;
    *trials = t;
    return SVO_OK;
}

// ------------------------------------------------------------------ trajectory output
int svo_pose_matrix3x4_inverse(const double* pose, double* out12) {
    if (!pose || !out12) return fail(SVO_ERR_ARG, "null argument");
    const svo::SE3 T{{pose[0], pose[1], pose[2], pose[3]}, {pose[4], pose[5], pose[6]}};
    const svo::SE3 Ti = svo::se3_inverse(T);  // Sophus SE3::inverse
    double R[3][3];
    svo::rotmat(Ti.q, R);  // SO3::matrix (Eigen toRotationMatrix)
    const double t[3] = {Ti.t.x, Ti.t.y, Ti.t.z};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out12[4 * r + c] = R[r][c];
        out12[4 * r + 3] = t[r];
    }
    return SVO_OK;
}

int svo_format_kitti_pose(const double* pose, char* buf, int32_t cap) {
    if (!buf || cap < 1) return fail(SVO_ERR_ARG, "null argument");
    double m[12];
    if (int r = svo_pose_matrix3x4_inverse(pose, m)) return r;
    int32_t o = 0;
    for (int i = 0; i < 12; ++i) {
        const int k = std::snprintf(buf + o, (size_t)(cap - o), i ? " %.6g" : "%.6g", m[i]);
        if (k < 0 || k >= cap - o) {
            buf[0] = 0;
            return fail(SVO_ERR_ARG, "buffer of %d bytes too short", cap);
        }
        o += k;
    }
    return SVO_OK;
}
}  // extern "C"
