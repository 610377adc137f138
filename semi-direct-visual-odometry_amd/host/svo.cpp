// svo.cpp — implementation of the C++ class-surface mirror (host/svo.hpp) over the C ABI.
#include <cstring>
#include "svo.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <iomanip>
#include <random>
#include <string>
#include <unordered_map>

namespace svo_amd {

static void check(int rc) {
    if (rc != SVO_OK) throw Error(rc, std::string("svo: ") + svo_last_error());
}

Context::Context(int device) { check(svo_ctx_create(device, &m_ctx)); }
Context::~Context() { svo_ctx_destroy(m_ctx); }

Vec2 PinholeCamera::project2d(const Vec3& p) const { return {fx * (p[0] / p[2]) + cx, fy * (p[1] / p[2]) + cy}; }
Vec3 PinholeCamera::inverseProject2d(const Vec2& px) const {
    Vec3 v{(px[0] - cx) / fx, (px[1] - cy) / fy, 1.0};
    const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    return {v[0] * (1.0 / n), v[1] * (1.0 / n), v[2] * (1.0 / n)};
}
bool PinholeCamera::isInFrame(const Vec2& p, double b) const {
    return p[0] >= b && p[1] >= b && p[0] < width - b && p[1] < height - b;
}

Vec2 PinholeCamera::rawPixel(const Vec2& p) const {
    const double x = (p[0] - cx) / fx, y = (p[1] - cy) / fy;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = (2.0 * x) * y;
    const double kr = 1.0 + ((d4 * r2 + d1) * r2 + d0) * r2;
    const double xd = (x * kr + d2 * xy2) + d3 * (r2 + 2.0 * x2);
    const double yd = (y * kr + d2 * (r2 + 2.0 * y2)) + d3 * xy2;
    return {fx * xd + cx, fy * yd + cy};
}
Vec2 PinholeCamera::undistortedPixel(const Vec2& raw) const {
    const double xd = (raw[0] - cx) / fx, yd = (raw[1] - cy) / fy;
    double x = xd, y = yd;
    for (int it = 0; it < SVO_UNDISTORT_POINT_ITERATIONS; ++it) {
        const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = (2.0 * x) * y;
        const double kr = 1.0 + ((d4 * r2 + d1) * r2 + d0) * r2;
        const double tx = d2 * xy2 + d3 * (r2 + 2.0 * x2), ty = d2 * (r2 + 2.0 * y2) + d3 * xy2;
        x = (xd - tx) / kr;
        y = (yd - ty) / kr;
    }
    return {fx * x + cx, fy * y + cy};
}
const svo_undistort_map* PinholeCamera::undistortMap(Context& ctx) const {
    if (!m_map || m_mapCtx != ctx.get()) {
        const svo_camera cam = c();
        const svo_distortion d{d0, d1, d2, d3, d4};
        svo_undistort_map* m = nullptr;
        check(svo_undistort_map_create(ctx.get(), &cam, &d, &m));
        m_map.reset(m, [](svo_undistort_map* q) { svo_undistort_map_destroy(q); });
        m_mapCtx = ctx.get();
    }
    return m_map.get();
}
std::vector<uint8_t> PinholeCamera::undistortImage(Context& ctx, const uint8_t* img) const {
    std::vector<uint8_t> out(img, img + (size_t)width * height);
    if (applyDistortion()) check(svo_undistort_images(ctx.get(), undistortMap(ctx), img, out.data(), 1));
    return out;
}

ImagePyramid::ImagePyramid(Context& ctx, std::size_t levels) : m_ctx(ctx), m_levels(levels) {}
ImagePyramid::ImagePyramid(Context& ctx, const uint8_t* img, int32_t w, int32_t h, std::size_t levels)
    : m_ctx(ctx), m_levels(levels) {
    createImagePyramid(img, w, h, levels);
}
ImagePyramid::ImagePyramid(Context& ctx, const ImageView& img, int32_t w, int32_t h, std::size_t levels)
    : m_ctx(ctx), m_levels(levels) {
    createImagePyramid(img, w, h, levels);
}
ImagePyramid::~ImagePyramid() { clear(); }
void ImagePyramid::createImagePyramid(const uint8_t* img, int32_t w, int32_t h, std::size_t levels,
                                      const svo_undistort_map* undistort) {
    clear();
    m_levels = levels;
    check(svo_pyramid_set_create(m_ctx.get(), 1, w, h, (int32_t)levels, &m_set));
    if (undistort) check(svo_pyramid_set_upload_undistort(m_set, 0, 1, img, undistort));
    else check(svo_pyramid_set_upload(m_set, 0, 1, img));
    check(svo_pyramid_set_build(m_set, 0, 1));
    check(svo_ctx_synchronize(m_ctx.get()));
}
void ImagePyramid::createImagePyramid(const ImageView& img, int32_t w, int32_t h, std::size_t levels,
                                      const svo_undistort_map* undistort) {
    clear();
    m_levels = levels;
    check(svo_pyramid_set_create(m_ctx.get(), 1, w, h, (int32_t)levels, &m_set));
    check(svo_pyramid_set_upload_format(m_set, 0, 1, img.data, &img.layout, undistort));
    check(svo_pyramid_set_build(m_set, 0, 1));
    check(svo_ctx_synchronize(m_ctx.get()));
}
std::array<int32_t, 2> ImagePyramid::getImageSizeAtLevel(std::size_t level) const {
    std::array<int32_t, 2> s{0, 0};
    if (m_set) check(svo_pyramid_level_size(m_set, (int32_t)level, &s[0], &s[1]));
    return s;
}
std::vector<uint8_t> ImagePyramid::getImageAtLevel(std::size_t level) const {
    auto s = getImageSizeAtLevel(level);
    std::vector<uint8_t> out((size_t)s[0] * s[1]);
    check(svo_pyramid_set_download(m_set, 0, (int32_t)level, 0, out.data()));
    return out;
}
std::vector<uint8_t> ImagePyramid::getGradientAtLevel(std::size_t level) const {
    auto s = getImageSizeAtLevel(level);
    std::vector<uint8_t> out((size_t)s[0] * s[1]);
    check(svo_pyramid_set_download(m_set, 0, (int32_t)level, 1, out.data()));
    return out;
}
void ImagePyramid::clear() {
    if (m_set) svo_pyramid_set_destroy(m_set);
    m_set = nullptr;
}

Feature::Feature(Frame* frame, const Vec2& px)
    : m_frame(frame), m_pixelPosition(px), m_bearingVec(frame->m_camera->inverseProject2d(px)) {}

static uint64_t nextFrameId() {
    static uint64_t frameCounter = 0;  // Frame::m_frameCounter
    return frameCounter++;
}

Frame::Frame(Context& ctx, std::shared_ptr<PinholeCamera> camera, const uint8_t* img, uint32_t maxImagePyramid,
             std::shared_ptr<Frame> lastKeyframe)
    : m_camera(std::move(camera)), m_imagePyramid(ctx, maxImagePyramid), m_lastKeyframe(std::move(lastKeyframe)) {
    m_id = nextFrameId();
    if (!img) throw std::runtime_error("Image Corrupted");  // src/frame.cpp:20-24
    m_imagePyramid.createImagePyramid(img, m_camera->width, m_camera->height, maxImagePyramid,
                                      m_camera->applyDistortion() ? m_camera->undistortMap(ctx) : nullptr);
}
Frame::Frame(Context& ctx, std::shared_ptr<PinholeCamera> camera, const ImageView& img, uint32_t maxImagePyramid,
             std::shared_ptr<Frame> lastKeyframe)
    : m_camera(std::move(camera)), m_imagePyramid(ctx, maxImagePyramid), m_lastKeyframe(std::move(lastKeyframe)) {
    m_id = nextFrameId();
    if (!img.data) throw std::runtime_error("Image Corrupted");  // src/frame.cpp:20-24
    m_imagePyramid.createImagePyramid(img, m_camera->width, m_camera->height, maxImagePyramid,
                                      m_camera->applyDistortion() ? m_camera->undistortMap(ctx) : nullptr);
}

ImageAlignment::ImageAlignment(Context& ctx, uint32_t patchSize, int32_t minLevel, int32_t maxLevel, uint32_t numParameters,
                               int32_t medianMode)
    : m_ctx(ctx), m_params{(int32_t)patchSize, minLevel, maxLevel, medianMode} {
    if (numParameters != 6) throw Error(SVO_ERR_ARG, "ImageAlignment: numParameters must be 6");
}

ImageAlignment::~ImageAlignment() {
    if (m_batch) svo_align_batch_destroy(m_batch);
}

double ImageAlignment::align(std::shared_ptr<Frame>& refFrame, std::shared_ptr<Frame>& curFrame) {
    if (refFrame->numberObservation() == 0) return 0;  // src/image_alignment.cpp:27-28
    const auto& kf = refFrame->m_lastKeyframe;
    const int32_t nr = (int32_t)refFrame->numberObservation(), nk = (int32_t)kf->numberObservation();
    m_px.clear(); m_br.clear(); m_pt.clear(); m_hp.clear();
    for (const auto* fr : {refFrame.get(), kf.get()})
        for (const auto& f : fr->m_features) {
            m_px.insert(m_px.end(), f->m_pixelPosition.begin(), f->m_pixelPosition.end());
            m_br.insert(m_br.end(), f->m_bearingVec.begin(), f->m_bearingVec.end());
            const Vec3 p = f->m_point ? f->m_point->m_position : Vec3{0, 0, 0};
            m_pt.insert(m_pt.end(), p.begin(), p.end());
            m_hp.push_back(f->m_point ? 1 : 0);
        }
    const svo_camera cam = refFrame->m_camera->c();
    const bool same_cam = m_batch && std::memcmp(&cam, &m_batchCam, sizeof(cam)) == 0;
    if (!same_cam || nr + nk > m_batchCap) {  // grow-only: a new batch only for a larger frame or another camera
        if (m_batch) svo_align_batch_destroy(m_batch);
        m_batch = nullptr;
        int32_t grow = same_cam ? 2 * m_batchCap : 1;
        if (m_params.median_mode == SVO_MEDIAN_REFERENCE)  // doubling must not cross the reference-mode limit
            grow = std::min(grow, SVO_REF_MAX_SLOTS / (m_params.patch_size * m_params.patch_size));
        const int32_t cap = std::max(nr + nk, grow);
        check(svo_align_batch_create(m_ctx.get(), &cam, &m_params, 1, cap, &m_batch));
        m_batchCap = cap;
        m_batchCam = cam;
    }
    double err = 0.0;
    check(svo_align_batch_set_pair(m_batch, 0, refFrame->m_imagePyramid.set(), 0, kf->m_imagePyramid.set(), 0,
                                   curFrame->m_imagePyramid.set(), 0, refFrame->m_absPose.data(), kf->m_absPose.data(),
                                   curFrame->m_absPose.data(), nr, nk, m_px.data(), m_br.data(), m_pt.data(),
                                   m_hp.data()));
    check(svo_align_batch_run(m_batch));
    check(svo_align_batch_results(m_batch, curFrame->m_absPose.data(), &err, &m_status));
    return err;
}

FeatureAlignment::FeatureAlignment(Context& ctx, uint32_t patchSize, int32_t level, uint32_t numParameters)
    : m_ctx(ctx), m_patchSize(patchSize) {
    if (numParameters != 3) throw Error(SVO_ERR_ARG, "FeatureAlignment: numParameters must be 3");
    if (level != 0) throw Error(SVO_ERR_ARG, "FeatureAlignment works on level 0 (src/feature_alignment.cpp:69)");
}

double FeatureAlignment::align(const std::shared_ptr<Feature>& refFeature, const std::shared_ptr<Frame>& curFrame,
                               Vec2& pixelPos) {
    svo_camera cam = curFrame->m_camera->c();
    double err = 0.0;
    check(svo_feature_align(m_ctx.get(), &cam, (int32_t)m_patchSize, refFeature->m_frame->m_imagePyramid.set(), nullptr,
                            0, curFrame->m_imagePyramid.set(), 0, 1, refFeature->m_pixelPosition.data(),
                            pixelPos.data(), &err, &m_status));
    return err;
}

// ------------------------------------------------------------------ FeatureSelection
FeatureSelection::FeatureSelection(Context& ctx, int32_t width, int32_t height, int32_t cellSize)
    : m_ctx(ctx), m_width(width), m_height(height), m_cellSize(cellSize) {
    check(svo_feature_grid_size(width, height, cellSize, &m_gridRows, &m_gridCols));
    m_occupancyGrid.assign((size_t)m_gridRows * m_gridCols, 0);
}

void FeatureSelection::emit(std::shared_ptr<Frame>& frame, const std::vector<double>& px, const std::vector<double>& resp,
                            int32_t n) {
    for (int32_t i = 0; i < n; ++i) {  // Feature(frame, px, response, angle 0, level 0, EDGE) (:68-71)
        auto f = std::make_shared<Feature>(frame.get(), Vec2{px[2 * i], px[2 * i + 1]});
        f->m_gradientMagnitude = resp[i];
        frame->m_features.push_back(std::move(f));
    }
}

void FeatureSelection::gradientMagnitudeWithSSC(std::shared_ptr<Frame>& frame, uint32_t detectionThreshold,
                                                uint32_t numberCandidate, bool useBucketing) {
    const int32_t cap = useBucketing ? m_gridRows * m_gridCols : m_width * m_height;
    std::vector<double> px(2 * (size_t)cap), resp(cap);
    int32_t n = 0;
    check(svo_feature_select_ssc(m_ctx.get(), frame->m_imagePyramid.set(), 0, (int32_t)detectionThreshold,
                                 (int32_t)numberCandidate, useBucketing ? 1 : 0, m_cellSize, m_occupancyGrid.data(), cap,
                                 px.data(), resp.data(), &n, nullptr));
    emit(frame, px, resp, n);
}

void FeatureSelection::gradientMagnitudeByValue(std::shared_ptr<Frame>& frame, uint32_t detectionThreshold,
                                                bool useBucketing) {
    if (!useBucketing) throw Error(SVO_ERR_ARG, "svo: gradientMagnitudeByValue without bucketing is not supported");
    const int32_t cap = m_gridRows * m_gridCols;
    std::vector<double> px(2 * (size_t)cap), resp(cap);
    int32_t n = 0;
    check(svo_feature_select_by_value(m_ctx.get(), frame->m_imagePyramid.set(), 0, (int32_t)detectionThreshold,
                                      m_cellSize, m_occupancyGrid.data(), cap, px.data(), resp.data(), &n));
    emit(frame, px, resp, n);
}

void FeatureSelection::setExistingFeatures(const std::vector<std::shared_ptr<Feature>>& features) {
    for (const auto& f : features) setCellInGridOccupancy(f->m_pixelPosition);
}

void FeatureSelection::setCellInGridOccupancy(const Vec2& location) {  // :276-282
    const uint32_t idx = location[0] / m_cellSize;
    const uint32_t idy = location[1] / m_cellSize;
    m_occupancyGrid[idy * m_gridCols + idx] = 1;
}

void FeatureSelection::resetGridOccupancy() { std::fill(m_occupancyGrid.begin(), m_occupancyGrid.end(), 0); }

// ------------------------------------------------------------------ BundleAdjustment
BundleAdjustment::BundleAdjustment(Context& ctx, std::shared_ptr<PinholeCamera> camera, int32_t level,
                                   uint32_t numParameters)
    : m_ctx(ctx), m_camera(std::move(camera)) {
    if (numParameters != 6 || level != 0) throw Error(SVO_ERR_ARG, "svo: BundleAdjustment(camera, 0, 6) only");
}

double BundleAdjustment::optimizePose(std::shared_ptr<Frame>& frame) {
    const std::size_t n = frame->numberObservation();
    if (n == 0) return 0;  // src/bundle_adjustment.cpp:37-38
    m_refVisibility.resize(n, 0);
    std::vector<double> bearing(3 * n), point(3 * n, 0.0);
    std::vector<uint8_t> has(n, 0);
    for (std::size_t k = 0; k < n; ++k) {
        const auto& f = frame->m_features[k];
        for (int i = 0; i < 3; ++i) bearing[3 * k + i] = f->m_bearingVec[i];
        if (f->m_point) {
            has[k] = 1;
            for (int i = 0; i < 3; ++i) point[3 * k + i] = f->m_point->m_position[i];
        }
    }
    const int32_t off[2] = {0, (int32_t)n};
    double err = 0.0;
    check(svo_pose_optimize(m_ctx.get(), 1, off, bearing.data(), point.data(), has.data(), m_refVisibility.data(),
                            frame->m_absPose.data(), &err, &m_status));
    return err;
}

// ------------------------------------------------------------------ DepthEstimator
void DepthEstimator::addKeyframe(const std::shared_ptr<Frame>& frame, double depthMean, double depthMin) {
    dropDeletedKeyframe();
    const int32_t kf = (int32_t)m_keyframes.size();
    m_keyframes.push_back(frame);
    for (const auto& f : frame->m_features) {
        if (f->m_point) continue;  // initializeFilters: features without a point only
        svo_depth_seed sd{};
        check(svo_depth_seed_init(depthMean, depthMin, &sd));  // MixedGaussianFilter (src/mixed_gaussian_filter.cpp:7-24)
        sd.px[0] = f->m_pixelPosition[0];
        sd.px[1] = f->m_pixelPosition[1];
        for (int i = 0; i < 3; ++i) sd.bearing[i] = f->m_bearingVec[i];
        sd.kf = kf;
        m_seeds.push_back(sd);
        m_features.push_back(f);
    }
}

std::vector<std::pair<std::shared_ptr<Feature>, std::shared_ptr<Point>>> DepthEstimator::updateFilters(
    const std::shared_ptr<Frame>& frame) {
    std::vector<std::pair<std::shared_ptr<Feature>, std::shared_ptr<Point>>> out;
    const int32_t n = (int32_t)m_seeds.size();
    if (n == 0) return out;
    const int32_t nk = (int32_t)m_keyframes.size();
    std::vector<const svo_pyramid_set*> sets(nk);
    std::vector<int32_t> frames(nk, 0);
    std::vector<double> poses(7 * (size_t)nk);
    for (int32_t k = 0; k < nk; ++k) {
        sets[k] = m_keyframes[k]->m_imagePyramid.set();
        for (int i = 0; i < 7; ++i) poses[7 * k + i] = m_keyframes[k]->m_absPose[i];
    }
    std::vector<int32_t> outcome(n), cand_seed(n);
    std::vector<double> cand_points(3 * (size_t)n);
    int32_t n_out = 0, n_cand = 0;
    const svo_camera cam = frame->m_camera->c();
    std::vector<svo_depth_seed> seeds = m_seeds;
    check(svo_depth_update(m_ctx.get(), &cam, nk, sets.data(), frames.data(), poses.data(), frame->m_imagePyramid.set(),
                           0, frame->m_absPose.data(), n, seeds.data(), &n_out, outcome.data(), cand_points.data(),
                           cand_seed.data(), &n_cand));
    for (int32_t j = 0; j < n_cand; ++j)
        out.emplace_back(m_features[cand_seed[j]],
                         std::make_shared<Point>(Point{{cand_points[3 * j], cand_points[3 * j + 1], cand_points[3 * j + 2]}}));
    std::vector<std::shared_ptr<Feature>> keep;  // survivors, order kept (remove_if, :300-308)
    for (int32_t i = 0; i < n; ++i)
        if (outcome[i] == SVO_DEPTH_NO_MATCH || outcome[i] == SVO_DEPTH_UPDATED) keep.push_back(m_features[i]);
    m_features.swap(keep);
    seeds.resize(n_out);
    m_seeds.swap(seeds);
    return out;
}

// ------------------------------------------------------------------ Map
Map::Map(Context& ctx, std::shared_ptr<PinholeCamera> camera, int32_t cellSize, uint64_t seed)
    : m_ctx(ctx), m_camera(std::move(camera)), m_cellSize(cellSize) {
    m_gridCols = (m_camera->width + cellSize - 1) / cellSize;  // src/map.cpp:222-248
    m_gridRows = (m_camera->height + cellSize - 1) / cellSize;
    const int32_t n = m_gridCols * m_gridRows;
    m_cellOrders.resize(n);
    for (int32_t i = 0; i < n; ++i) m_cellOrders[i] = i;
    std::mt19937_64 rng(seed);
    std::shuffle(m_cellOrders.begin(), m_cellOrders.end(), rng);
    m_cellVisited.assign(n, 0);
}

void Map::reprojectMap(const std::shared_ptr<Frame>& refFrame, std::shared_ptr<Frame>& curFrame,
                       std::vector<std::pair<std::shared_ptr<Frame>, int32_t>>& overlapKeyFrames) {
    if (!refFrame->m_lastKeyframe) throw Error(SVO_ERR_ARG, "svo: reprojectMap needs refFrame->m_lastKeyframe");
    const std::shared_ptr<Frame> kfs[2] = {refFrame, refFrame->m_lastKeyframe};
    std::vector<std::shared_ptr<Feature>> feats;
    int32_t off[3] = {0, 0, 0};
    for (int k = 0; k < 2; ++k) {
        feats.insert(feats.end(), kfs[k]->m_features.begin(), kfs[k]->m_features.end());
        off[k + 1] = (int32_t)feats.size();
    }
    std::vector<std::shared_ptr<Point>> points;
    std::unordered_map<const Point*, int32_t> index;
    std::vector<int32_t> featPoint(std::max<size_t>(feats.size(), 1), -1);
    for (size_t i = 0; i < feats.size(); ++i) {
        const auto& pt = feats[i]->m_point;
        if (!pt) continue;
        auto it = index.emplace(pt.get(), (int32_t)points.size());
        if (it.second) points.push_back(pt);
        featPoint[i] = it.first->second;
    }
    const size_t np = std::max<size_t>(points.size(), 1);
    std::vector<double> pos(3 * np, 0.0);
    std::vector<uint32_t> type(np, 0);
    std::vector<uint64_t> last(np, 0);
    for (size_t i = 0; i < points.size(); ++i) {
        for (int j = 0; j < 3; ++j) pos[3 * i + j] = points[i]->m_position[j];
        type[i] = (uint32_t)points[i]->m_type;
        last[i] = points[i]->m_lastProjectedKFId;
    }
    const int32_t nCells = (int32_t)m_cellOrders.size();
    std::vector<int32_t> selFeat(nCells), selCell(nCells);
    std::vector<double> selPx(2 * (size_t)nCells);
    int32_t overlap[2] = {0, 0}, nSel = 0, matches = 0, trials = 0;
    const svo_camera cam = m_camera->c();
    check(svo_map_reproject_plan(&cam, m_cellSize, nCells, m_cellOrders.data(), curFrame->m_absPose.data(),
                                 curFrame->m_id, 2, off, featPoint.data(), (int32_t)points.size(), pos.data(),
                                 type.data(), last.data(), overlap, &nSel, selFeat.data(), selCell.data(),
                                 selPx.data(), &matches, &trials));
    for (size_t i = 0; i < points.size(); ++i) points[i]->m_lastProjectedKFId = last[i];
    for (int k = 0; k < 2; ++k) overlapKeyFrames.emplace_back(kfs[k], overlap[k]);
    m_matches = (uint32_t)matches;
    m_trials = (uint32_t)trials;
    if (nSel == 0) return;
    std::vector<const svo_pyramid_set*> sets(nSel);
    std::vector<int32_t> frames(nSel, 0), status(nSel);
    std::vector<double> refPx(2 * (size_t)nSel), err(nSel);
    for (int32_t i = 0; i < nSel; ++i) {
        const auto& f = feats[selFeat[i]];
        sets[i] = f->m_frame->m_imagePyramid.set();
        refPx[2 * i] = f->m_pixelPosition[0];
        refPx[2 * i + 1] = f->m_pixelPosition[1];
    }
    check(svo_feature_align_multi(m_ctx.get(), &cam, 7, sets.data(), frames.data(), curFrame->m_imagePyramid.set(), 0,
                                  nSel, refPx.data(), selPx.data(), err.data(), status.data()));
    for (int32_t i = 0; i < nSel; ++i) {  // src/map.cpp:558-569
        const auto& point = feats[selFeat[i]]->m_point;
        point->m_succeededProjection++;
        if (point->m_type == Point::PointType::UNKNOWN && point->m_succeededProjection > 10)
            point->m_type = Point::PointType::GOOD;
        auto feature = std::make_shared<Feature>(curFrame.get(), Vec2{selPx[2 * i], selPx[2 * i + 1]});
        curFrame->m_features.push_back(feature);
        feature->m_point = point;
        point->m_features.push_back(feature);
        m_cellVisited[selCell[i]] = 1;
    }
}

void Map::addNewCandidate(const std::shared_ptr<Feature>& feature, const std::shared_ptr<Point>& point) {
    point->m_type = Point::PointType::CANDIDATE;  // src/map.cpp:586-593
    m_candidates.push_back({feature, point, false});
}

void Map::addCandidateToFrame(std::shared_ptr<Frame>& frame) {
    const int32_t n = (int32_t)m_candidates.size();
    if (n == 0) return;
    std::vector<double> pos(3 * (size_t)n), px0(2 * (size_t)n);
    for (int32_t i = 0; i < n; ++i)
        for (int j = 0; j < 3; ++j) pos[3 * i + j] = m_candidates[i].point->m_position[j];
    const svo_camera cam = m_camera->c();
    check(svo_world2image(&cam, frame->m_absPose.data(), n, pos.data(), px0.data()));
    const double w = frame->m_camera->width, h = frame->m_camera->height;
    std::vector<int32_t> elig, cells;
    for (int32_t i = 0; i < n; ++i) {  // isInFrame(px, 3) and a free cell (:600-606)
        const double x = px0[2 * i], y = px0[2 * i + 1];
        if (!(x >= 3 && y >= 3 && x < w - 3 && y < h - 3)) continue;
        const int32_t cell = (int32_t)y / m_cellSize * m_gridCols + (int32_t)x / m_cellSize;
        if (m_cellVisited[cell]) continue;
        elig.push_back(i);
        cells.push_back(cell);
    }
    const int32_t ne = (int32_t)elig.size();
    if (ne == 0) return;
    std::vector<const svo_pyramid_set*> sets(ne);
    std::vector<int32_t> frames(ne, 0), status(ne);
    std::vector<double> refPx(2 * (size_t)ne), px(2 * (size_t)ne), err(ne);
    for (int32_t j = 0; j < ne; ++j) {
        const auto& f = m_candidates[elig[j]].feature;
        sets[j] = f->m_frame->m_imagePyramid.set();
        refPx[2 * j] = f->m_pixelPosition[0];
        refPx[2 * j + 1] = f->m_pixelPosition[1];
        px[2 * j] = px0[2 * elig[j]];
        px[2 * j + 1] = px0[2 * elig[j] + 1];
    }
    check(svo_feature_align_multi(m_ctx.get(), &cam, 7, sets.data(), frames.data(), frame->m_imagePyramid.set(), 0, ne,
                                  refPx.data(), px.data(), err.data(), status.data()));
    for (int32_t j = 0; j < ne; ++j) {  // list order: a cell taken earlier in this loop is skipped (:607-624)
        if (m_cellVisited[cells[j]] || !(err[j] < 50.0)) continue;
        Candidate& c = m_candidates[elig[j]];
        auto feature = std::make_shared<Feature>(frame.get(), Vec2{px[2 * j], px[2 * j + 1]});
        frame->m_features.push_back(feature);
        c.point->m_features.push_back(c.feature);
        c.point->m_features.push_back(feature);
        c.feature->m_point = c.point;
        feature->m_point = c.point;
        c.matched = true;
        m_cellVisited[cells[j]] = 1;
    }
    removeMatchedCandidate();  // (:626)
}

void Map::removeMatchedCandidate() {  // src/map.cpp:629-634
    m_candidates.erase(std::remove_if(m_candidates.begin(), m_candidates.end(), [](const Candidate& c) { return c.matched; }),
                       m_candidates.end());
}

// ------------------------------------------------------------------ windowed bundle adjustment
void Point::removeFrame(const Frame* frame) {  // src/point.cpp:40-49
    m_features.erase(std::remove_if(m_features.begin(), m_features.end(),
                                    [frame](const std::weak_ptr<Feature>& w) {
                                        const auto f = w.lock();
                                        return f && f->m_frame == frame;
                                    }),
                     m_features.end());
}

void Frame::removeFeature(const std::shared_ptr<Feature>& feature) {  // src/frame.cpp:39-49
    m_features.erase(std::remove(m_features.begin(), m_features.end(), feature), m_features.end());
}

void removePoint(std::shared_ptr<Point>& point) {  // src/map.cpp:76-87
    const std::shared_ptr<Point> keep = point;  // (`point` may be the m_point of a feature about to leave its frame)
    for (auto& w : keep->m_features)
        if (const auto feature = w.lock()) feature->m_frame->removeFeature(feature);
    keep->m_features.clear();
    keep->m_type = Point::PointType::DELETED;
    point = nullptr;
}

void removeFeature(std::shared_ptr<Feature>& feature) {  // src/map.cpp:89-110
    if (feature->m_point == nullptr) return;
    if (feature->m_point->numberObservation() <= 2) {
        removePoint(feature->m_point);
        return;
    }
    feature->m_point->removeFrame(feature->m_frame);
    feature->m_frame->removeFeature(feature);
    feature = nullptr;
}

BundleAdjustment::WindowResult BundleAdjustment::adjust(const std::vector<Frame*>& frames, const std::vector<uint8_t>& fixed,
                                                        const std::vector<std::shared_ptr<Point>>& points,
                                                        std::vector<Edge>& edges, double reprojectionError,
                                                        int32_t structureIterations) {
    if (frames.size() - (std::size_t)std::count_if(fixed.begin(), fixed.end(), [](uint8_t f) { return f != 0; }) > SVO_BA_MAX_FRAMES)
        throw Error(SVO_ERR_ARG, "svo: bundle adjustment over more than 16 frames free to move");
    const int32_t frameOff[2] = {0, (int32_t)frames.size()}, pointOff[2] = {0, (int32_t)points.size()},
                  obsOff[2] = {0, (int32_t)edges.size()};
    std::vector<double> poses(7 * frames.size()), pos(3 * points.size()), px(2 * edges.size()), chi2(edges.size());
    std::vector<int32_t> of(edges.size()), op(edges.size());
    for (std::size_t i = 0; i < frames.size(); ++i) std::copy(frames[i]->m_absPose.begin(), frames[i]->m_absPose.end(), &poses[7 * i]);
    for (std::size_t j = 0; j < points.size(); ++j) std::copy(points[j]->m_position.begin(), points[j]->m_position.end(), &pos[3 * j]);
    for (std::size_t k = 0; k < edges.size(); ++k) {
        of[k] = edges[k].frame;
        op[k] = edges[k].point;
        px[2 * k] = edges[k].feature->m_pixelPosition[0];
        px[2 * k + 1] = edges[k].feature->m_pixelPosition[1];
    }
    const svo_camera cam = m_camera->c();
    WindowResult res;
    int32_t iterations = 0;
    check(svo_bundle_adjust(m_ctx.get(), &cam, 1, frameOff, pointOff, obsOff, poses.data(), fixed.data(), pos.data(),
                            of.data(), op.data(), px.data(), reprojectionError, 10, structureIterations, chi2.data(),
                            &res.initError, &res.finalError, &iterations, &m_status, nullptr));
    for (std::size_t i = 0; i < frames.size(); ++i)
        if (!fixed[i]) std::copy(&poses[7 * i], &poses[7 * i] + 7, frames[i]->m_absPose.begin());
    for (std::size_t j = 0; j < points.size(); ++j) std::copy(&pos[3 * j], &pos[3 * j] + 3, points[j]->m_position.begin());
    const double chiSquaredError = reprojectionError * reprojectionError;
    for (std::size_t k = 0; k < edges.size(); ++k)  // (:461-476, :598-609)
        if (chi2[k] > chiSquaredError) {
            removeFeature(edges[k].feature);
            ++res.removed;
        }
    return res;
}

BundleAdjustment::WindowResult BundleAdjustment::twoViewBA(std::shared_ptr<Frame>& fstFrame, std::shared_ptr<Frame>& secFrame,
                                                           double reprojectionError) {
    std::vector<std::shared_ptr<Point>> points;
    std::vector<Edge> edges;
    for (auto& feature : fstFrame->m_features) {
        if (feature->m_point == nullptr) continue;
        std::shared_ptr<Feature> inSec;  // Point::findFeature(secFrame)
        for (auto& f : secFrame->m_features)
            if (f->m_point == feature->m_point) { inSec = f; break; }
        if (!inSec) throw Error(SVO_ERR_ARG, "svo: a point of the first frame is not observed in the second frame");
        edges.push_back({0, (int32_t)points.size(), feature});
        edges.push_back({1, (int32_t)points.size(), inSec});
        points.push_back(feature->m_point);
    }
    return adjust({fstFrame.get(), secFrame.get()}, {1, 0}, points, edges, reprojectionError, 0);
}

BundleAdjustment::WindowResult BundleAdjustment::localBA(std::vector<std::shared_ptr<Frame>>& keyFrames, double reprojectionError) {
    std::vector<Frame*> frames;
    for (auto& kf : keyFrames) frames.push_back(kf.get());
    const std::size_t nKey = frames.size();
    std::vector<std::shared_ptr<Point>> points;
    for (auto& kf : keyFrames)
        for (auto& feature : kf->m_features) {
            const auto& p = feature->m_point;
            if (p != nullptr && p->numberObservation() > 1 && std::find(points.begin(), points.end(), p) == points.end())
                points.push_back(p);
        }
    std::vector<Edge> edges;
    for (std::size_t j = 0; j < points.size(); ++j)
        for (auto& w : points[j]->m_features) {
            const auto feature = w.lock();
            if (!feature) throw Error(SVO_ERR_STATE, "svo: a point is observed by a feature no frame holds");
            auto it = std::find(frames.begin(), frames.end(), feature->m_frame);
            if (it == frames.end()) {  // a neighbour keyframe: fixed (:532-540)
                frames.push_back(feature->m_frame);
                it = frames.end() - 1;
            }
            edges.push_back({(int32_t)(it - frames.begin()), (int32_t)j, feature});
        }
    std::vector<uint8_t> fixed(frames.size(), 0);
    std::fill(fixed.begin() + (std::ptrdiff_t)nKey, fixed.end(), (uint8_t)1);
    return adjust(frames, fixed, points, edges, reprojectionError, 10);
}

// ------------------------------------------------------------------ two-view map initialisation
static void matched_pixels(const Frame& ref, const Frame& cur, std::vector<double>& refPx, std::vector<double>& curPx) {
    const std::size_t n = ref.numberObservation();
    if (cur.numberObservation() != n) throw Error(SVO_ERR_ARG, "svo: ref and cur frames hold different feature counts");
    refPx.resize(2 * n);
    curPx.resize(2 * n);
    for (std::size_t i = 0; i < n; ++i)
        for (int j = 0; j < 2; ++j) {
            refPx[2 * i + j] = ref.m_features[i]->m_pixelPosition[j];
            curPx[2 * i + j] = cur.m_features[i]->m_pixelPosition[j];
        }
}

void algorithm::triangulate3DWorldPoints(Context& ctx, const std::shared_ptr<Frame>& refFrame,
                                         const std::shared_ptr<Frame>& curFrame, std::vector<Vec3>& pointsWorld) {
    std::vector<double> refPx, curPx;
    matched_pixels(*refFrame, *curFrame, refPx, curPx);
    const int32_t n = (int32_t)refFrame->numberObservation();
    const int32_t off[2] = {0, n};
    const svo_camera cam = refFrame->m_camera->c();
    pointsWorld.resize((std::size_t)n);
    check(svo_triangulate_dlt(ctx.get(), &cam, 1, off, refFrame->m_absPose.data(), curFrame->m_absPose.data(),
                              refPx.data(), curPx.data(), n ? pointsWorld[0].data() : nullptr));
}

TwoViewResult initializeTwoView(Context& ctx, std::shared_ptr<Frame>& refFrame, std::shared_ptr<Frame>& curFrame,
                                const std::array<double, 9>& E, double mapScale, int32_t cellPixelSize) {
    std::vector<double> refPx, curPx;
    matched_pixels(*refFrame, *curFrame, refPx, curPx);
    const int32_t n = (int32_t)refFrame->numberObservation();
    const int32_t off[2] = {0, n};
    const svo_camera cam = refFrame->m_camera->c();
    const std::size_t cap = n ? (std::size_t)n : 1;
    std::vector<double> pointsWorld(3 * cap);
    std::vector<uint8_t> valid(cap);
    std::vector<int32_t> survivor(cap);
    double F[9], median = 0.0;
    int32_t nValid = 0;
    TwoViewResult res;
    Pose curPose = curFrame->m_absPose;
    check(svo_two_view_init(ctx.get(), &cam, 1, off, E.data(), refFrame->m_absPose.data(), mapScale, cellPixelSize,
                            refPx.data(), curPx.data(), F, res.counts.data(), &res.winner, curPose.data(), &median,
                            &nValid, pointsWorld.data(), valid.data(), survivor.data(), nullptr));
    for (int32_t i = 0; i < n; ++i) {  // sampsonCorrection (src/algorithm.cpp:233-234)
        refFrame->m_features[i]->m_pixelPosition = {refPx[2 * i], refPx[2 * i + 1]};
        curFrame->m_features[i]->m_pixelPosition = {curPx[2 * i], curPx[2 * i + 1]};
    }
    res.medianDepth = median;
    if (res.winner < 0) return res;  // recoverPose failed (src/system.cpp:152-156)
    res.ok = true;
    curFrame->m_absPose = curPose;
    for (int32_t k = 0; k < nValid; ++k) {  // (:201-209)
        const int32_t i = survivor[k];
        auto point = std::make_shared<Point>(Point{{pointsWorld[3 * i], pointsWorld[3 * i + 1], pointsWorld[3 * i + 2]}});
        refFrame->m_features[i]->m_point = point;
        curFrame->m_features[i]->m_point = point;
        point->m_features.push_back(refFrame->m_features[i]);
        point->m_features.push_back(curFrame->m_features[i]);
    }
    for (auto* fr : {refFrame.get(), curFrame.get()})  // (:217-223)
        fr->m_features.erase(std::remove_if(fr->m_features.begin(), fr->m_features.end(),
                                            [](const auto& feature) { return feature->m_point == nullptr; }),
                             fr->m_features.end());
    res.numPoints = (std::size_t)nValid;
    return res;
}

// ------------------------------------------------------------------ sparse optical flow
bool algorithm::computeOpticalFlowSparse(Context& ctx, std::shared_ptr<Frame>& refFrame, std::shared_ptr<Frame>& curFrame,
                                         uint32_t patchSize, double disparityThreshold) {
    const std::size_t n = refFrame->numberObservation();
    const std::size_t cap = n ? n : 1;
    std::vector<double> refPx(2 * cap), curPx(2 * cap);
    for (std::size_t i = 0; i < n; ++i)
        for (int j = 0; j < 2; ++j) refPx[2 * i + j] = curPx[2 * i + j] = refFrame->m_features[i]->m_pixelPosition[j];
    std::vector<uint8_t> status(cap, 0);
    const int32_t off[2] = {0, (int32_t)n}, frames[2] = {0, 0};
    double medianDisparity = 0.0;
    check(svo_klt_track(ctx.get(), refFrame->m_imagePyramid.set(), curFrame->m_imagePyramid.set(), 1, frames, off,
                        refPx.data(), curPx.data(), (int32_t)patchSize, 3, 30, 1e-4, 1e-4, status.data(), nullptr,
                        &medianDisparity));
    for (std::size_t i = 0; i < n; ++i)
        if (status[i]) {  // (:68-73)
            auto feature = std::make_shared<Feature>(curFrame.get(), Vec2{curPx[2 * i], curPx[2 * i + 1]});
            feature->m_gradientMagnitude = 0.0;
            curFrame->m_features.push_back(feature);
        }
    if (medianDisparity < disparityThreshold) return false;  // (:81-84)
    std::size_t cnt = 0;
    refFrame->m_features.erase(std::remove_if(refFrame->m_features.begin(), refFrame->m_features.end(),
                                              [&](const auto& feature) { return !(feature != nullptr && status[cnt++] == 1); }),
                               refFrame->m_features.end());
    return true;
}

// ------------------------------------------------------------------ essential-matrix RANSAC
bool algorithm::computeEssentialMatrix(Context& ctx, std::shared_ptr<Frame>& refFrame, std::shared_ptr<Frame>& curFrame,
                                       double reproError, uint32_t thresholdCorrespondingPoints, std::array<double, 9>& E,
                                       uint64_t seed) {
    std::vector<double> refPx, curPx;
    matched_pixels(*refFrame, *curFrame, refPx, curPx);
    const int32_t n = (int32_t)refFrame->numberObservation();
    const int32_t off[2] = {0, n};
    const svo_camera cam = refFrame->m_camera->c();
    std::vector<uint8_t> status(n ? (std::size_t)n : 1, 0);
    int32_t nInliers = 0, iterations = 0, best[2] = {-1, -1}, code = 0;
    check(svo_essential_ransac(ctx.get(), &cam, 1, off, refPx.data(), curPx.data(), reproError, 0.999, 1000, seed,
                               E.data(), status.data(), &nInliers, &iterations, best, &code, nullptr, nullptr));
    for (auto* frame : {&refFrame, &curFrame}) {  // (:140-161) the rejected matches leave both frames, order kept
        std::size_t cnt = 0;
        auto& features = (*frame)->m_features;
        features.erase(std::remove_if(features.begin(), features.end(), [&](const auto&) { return status[cnt++] == 0; }),
                       features.end());
    }
    return refFrame->numberObservation() > thresholdCorrespondingPoints &&
           curFrame->numberObservation() > thresholdCorrespondingPoints;  // (:166-170)
}

// ------------------------------------------------------------------ pose algebra, Frame helpers (System's host side)
// The operation order below is the Python mirror's (core.py _quat_rotate / _quat_mul / pose_compose / pose_inverse):
// with -ffp-contract=off both mirrors form the same bits.
static Vec3 cross3(const double* a, const Vec3& b) {
    return {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
}
static Vec3 quatRotate(const double* q, const Vec3& v) {  // Eigen's _transformVector
    Vec3 u = cross3(q, v);
    for (double& x : u) x = x + x;
    const Vec3 c = cross3(q, u);
    return {(v[0] + q[3] * u[0]) + c[0], (v[1] + q[3] * u[1]) + c[1], (v[2] + q[3] * u[2]) + c[2]};
}
static double norm3(const Vec3& d) { return std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]); }

Pose poseInverse(const Pose& p) {
    const double qi[4] = {p[0] * -1.0, p[1] * -1.0, p[2] * -1.0, p[3] * 1.0};
    const Vec3 t = quatRotate(qi, {p[4], p[5], p[6]});
    return {qi[0], qi[1], qi[2], qi[3], -t[0], -t[1], -t[2]};
}

Pose poseCompose(const Pose& a, const Pose& b) {
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    const double q[4] = {aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                         aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz};
    const double n = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const Vec3 t = quatRotate(a.data(), {b[4], b[5], b[6]});
    return {q[0] / n, q[1] / n, q[2] / n, q[3] / n, a[4] + t[0], a[5] + t[1], a[6] + t[2]};
}

uint32_t Frame::numberObservationWithPoints() const {
    uint32_t n = 0;
    for (const auto& f : m_features) n += f->m_point != nullptr;
    return n;
}
Vec3 Frame::world2camera(const Vec3& p) const {
    const Vec3 r = quatRotate(m_absPose.data(), p);
    return {r[0] + m_absPose[4], r[1] + m_absPose[5], r[2] + m_absPose[6]};
}
Vec3 Frame::cameraInWorld() const {
    const double qi[4] = {m_absPose[0] * -1.0, m_absPose[1] * -1.0, m_absPose[2] * -1.0, m_absPose[3] * 1.0};
    const Vec3 r = quatRotate(qi, {m_absPose[4], m_absPose[5], m_absPose[6]});
    return {-r[0], -r[1], -r[2]};
}
bool Frame::isVisible(const Vec3& p) const {
    const Vec3 c = world2camera(p);
    if (c[2] < 0.0) return false;
    return m_camera->isInFrame(m_camera->project2d(c));
}

Pose algorithm::computeRelativePose(const std::shared_ptr<Frame>& refFrame, const std::shared_ptr<Frame>& curFrame) {
    return poseCompose(curFrame->m_absPose, poseInverse(refFrame->m_absPose));
}
void algorithm::normalizedDepthCamera(const std::shared_ptr<Frame>& frame, std::vector<double>& out) {
    out.resize(frame->numberObservation());
    for (std::size_t i = 0; i < out.size(); ++i) {
        if (!frame->m_features[i]->m_point) throw Error(SVO_ERR_ARG, "svo: normalizedDepthCamera: a feature without a point");
        out[i] = norm3(frame->world2camera(frame->m_features[i]->m_point->m_position));
    }
}
double algorithm::computeMedian(const std::vector<double>& input) {
    std::vector<double> vec(input);
    if (vec.empty()) return std::nan("");
    const auto middleSize = vec.size() / 2;
    std::nth_element(vec.begin(), vec.begin() + (std::ptrdiff_t)middleSize, vec.end());
    return vec.size() % 2 != 0 ? vec[middleSize] : (vec[middleSize - 1] + vec[middleSize]) / 2.0;
}
uint32_t algorithm::computeNumberProjectedPoints(const std::shared_ptr<Frame>& curFrame) {
    const Pose rel = computeRelativePose(curFrame->m_lastKeyframe, curFrame);
    const Vec3 C = curFrame->cameraInWorld();
    uint32_t cnt = 0;
    for (const auto& f : curFrame->m_features) {
        if (!f->m_point) continue;
        const Vec3& X = f->m_point->m_position;
        const double depthNorm = norm3({X[0] - C[0], X[1] - C[1], X[2] - C[2]});
        const Vec3 r = quatRotate(rel.data(), {f->m_bearingVec[0] * depthNorm, f->m_bearingVec[1] * depthNorm,
                                               f->m_bearingVec[2] * depthNorm});
        if (curFrame->m_camera->isInFrame(curFrame->m_camera->project2d({r[0] + rel[4], r[1] + rel[5], r[2] + rel[6]}), 5.0))
            ++cnt;
    }
    return cnt;
}

// ------------------------------------------------------------------ Map: keyframes
void Map::getCloseKeyframes(const std::shared_ptr<Frame>& frame,
                            std::vector<std::pair<std::shared_ptr<Frame>, double>>& closeKeyframes) const {
    for (auto it = m_keyFrames.rbegin(); it != m_keyFrames.rend(); ++it) {
        const auto& keyFrame = *it;
        if (keyFrame == frame) continue;
        for (const auto& feature : keyFrame->m_features) {
            if (!feature->m_point || !frame->isVisible(feature->m_point->m_position)) continue;
            closeKeyframes.emplace_back(keyFrame, norm3({frame->m_absPose[4] - keyFrame->m_absPose[4],
                                                         frame->m_absPose[5] - keyFrame->m_absPose[5],
                                                         frame->m_absPose[6] - keyFrame->m_absPose[6]}));
            break;
        }
    }
}
void Map::getClosestKeyframe(const std::shared_ptr<Frame>& frame, std::shared_ptr<Frame>& closestKeyframe) const {
    std::vector<std::pair<std::shared_ptr<Frame>, double>> close;
    getCloseKeyframes(frame, close);
    closestKeyframe = nullptr;
    double minDistance = std::numeric_limits<double>::max();
    for (const auto& e : close)
        if (e.first != frame && e.second < minDistance) {
            minDistance = e.second;
            closestKeyframe = e.first;
        }
}
void Map::getFurthestKeyframe(const Vec3& pos, std::shared_ptr<Frame>& furthestKeyframe) const {
    double maxDistance = 0.0;
    for (const auto& frame : m_keyFrames) {
        const Vec3 c = frame->cameraInWorld();
        const double dist = norm3({c[0] - pos[0], c[1] - pos[1], c[2] - pos[2]});
        if (dist > maxDistance) {
            maxDistance = dist;
            furthestKeyframe = frame;
        }
    }
}
void Map::removeFrame(const std::shared_ptr<Frame>& frame) {
    const auto it = std::find(m_keyFrames.begin(), m_keyFrames.end(), frame);
    if (it == m_keyFrames.end()) throw Error(SVO_ERR_ARG, "svo: removeFrame: not a keyframe of this map");
    for (auto& feature : frame->m_features)
        if (feature->m_point) {
            feature->m_point->removeFrame(feature->m_frame);
            feature->m_point = nullptr;
        }
    frame->m_features.clear();
    frame->m_lastKeyframe = nullptr;
    m_keyFrames.erase(it);
    m_candidates.erase(std::remove_if(m_candidates.begin(), m_candidates.end(),
                                      [&](const Candidate& c) { return c.feature->m_frame == frame.get(); }),
                       m_candidates.end());
}

// ------------------------------------------------------------------ DepthEstimator: frames in, keyframes out
void DepthEstimator::reset() {
    m_keyframes.clear();
    m_features.clear();
    m_seeds.clear();
    m_deletedKeyframe = nullptr;
}
void DepthEstimator::dropDeletedKeyframe() {
    const std::shared_ptr<Frame> frame = std::move(m_deletedKeyframe);
    m_deletedKeyframe = nullptr;
    if (!frame) return;
    std::vector<int32_t> remap(m_keyframes.size(), -1);
    std::vector<std::shared_ptr<Frame>> kept;
    for (std::size_t k = 0; k < m_keyframes.size(); ++k)
        if (m_keyframes[k] != frame) {
            remap[k] = (int32_t)kept.size();
            kept.push_back(m_keyframes[k]);
        }
    std::vector<std::shared_ptr<Feature>> features;
    std::vector<svo_depth_seed> seeds;
    for (std::size_t i = 0; i < m_seeds.size(); ++i)
        if (m_features[i]->m_frame != frame.get()) {
            features.push_back(m_features[i]);
            seeds.push_back(m_seeds[i]);
            seeds.back().kf = remap[(std::size_t)m_seeds[i].kf];
        }
    m_keyframes.swap(kept);
    m_features.swap(features);
    m_seeds.swap(seeds);
}
void DepthEstimator::addFrame(const std::shared_ptr<Frame>& frame) {
    dropDeletedKeyframe();
    for (auto& c : updateFilters(frame))
        if (m_map) m_map->addNewCandidate(c.first, c.second);
}

// ------------------------------------------------------------------ System
System::System(Context& ctx, const Config& c)
    : m_ctx(ctx), m_config(c),
      m_camera(std::make_shared<PinholeCamera>(PinholeCamera{c.m_imgWidth, c.m_imgHeight, c.m_fx, c.m_fy, c.m_cx, c.m_cy,
                                                             c.m_d0, c.m_d1, c.m_d2, c.m_d3, c.m_d4})),
      m_alignment(ctx, c.m_patchSizeImageAlignment, c.m_minLevelImagePyramid, c.m_maxLevelImagePyramid, 6, c.m_medianMode),
      m_featureSelector(ctx, c.m_imgWidth, c.m_imgHeight, c.m_cellPixelSize),
      m_map(ctx, m_camera, c.m_cellPixelSize, c.m_mapCellSeed), m_depthEstimator(ctx, &m_map),
      m_bundler(ctx, m_camera, 0, 6) {}

template <class F> void System::timed(const char* name, F&& fn) {
    if (!m_instrument) {
        fn();
        return;
    }
    const auto t0 = std::chrono::steady_clock::now();
    fn();
    m_timings[name] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

template <class F> void System::runBA(const std::vector<std::shared_ptr<Frame>>& frames, F&& fn) {
    if (!m_instrument) {
        fn();
        return;
    }
    std::vector<std::vector<std::shared_ptr<Feature>>> before;
    for (const auto& fr : frames) before.push_back(fr->m_features);
    timed("ba", fn);
    for (std::size_t k = 0; k < frames.size(); ++k)
        for (std::size_t i = 0; i < before[k].size(); ++i)
            if (std::find(frames[k]->m_features.begin(), frames[k]->m_features.end(), before[k][i]) == frames[k]->m_features.end())
                m_baRemoved.emplace_back(frames[k]->m_id, i);
}

bool System::addImage(const uint8_t* img, uint64_t timestamp) {
    if (m_config.m_pixelFormat == SVO_PIXEL_GRAY8) return addFrame(img, timestamp);
    return addFrame(ImageView{img, svo_image_layout{m_config.m_pixelFormat, m_config.m_gray16Shift, 0, 0}}, timestamp);
}

bool System::addImage(const ImageView& img, uint64_t timestamp) { return addFrame(img, timestamp); }

template <class Image> bool System::addFrame(const Image& img, uint64_t timestamp) {
    if (m_instrument) {
        m_timings.clear();
        m_baRemoved.clear();
    }
    timed("frame", [&] {
        m_curFrame = std::make_shared<Frame>(m_ctx, m_camera, img, (uint32_t)m_config.m_maxLevelImagePyramid + 1, m_activeKeyframe);
    });
    m_curFrame->m_timestamp = timestamp;
    m_allFrames.push_back(m_curFrame);
    Result res = Result::Failed;
    if (m_systemStatus == Status::Procese_New_Frame) res = processNewFrame();
    else if (m_systemStatus == Status::Process_Second_Frame) res = processSecondFrame();
    else if (m_systemStatus == Status::Process_First_Frame) res = processFirstFrame();
    else if (m_systemStatus == Status::Process_Relocalization) {
        std::shared_ptr<Frame> closestKeyframe;
        m_map.getClosestKeyframe(m_curFrame, closestKeyframe);
        res = relocalizeFrame(closestKeyframe);
    }
    if (m_refFrame != nullptr) m_predictionRelativePose = algorithm::computeRelativePose(m_refFrame, m_curFrame);
    m_lastResult = res;
    if (res == Result::Failed) return false;
    m_refFrame = m_curFrame;
    return true;
}

void System::select(std::shared_ptr<Frame>& frame) {
    timed("select", [&] {
        m_featureSelector.gradientMagnitudeWithSSC(frame, m_config.m_thresholdGradientMagnitude,
                                                   m_config.m_desiredDetectedPointsForInitialization, true);
    });
}

System::Result System::processFirstFrame() {
    select(m_curFrame);
    if (m_curFrame->numberObservation() < m_config.m_minDetectedPointsSuccessInitialization) return Result::Failed;
    m_curFrame->setKeyframe();
    m_activeKeyframe = m_curFrame;
    m_map.addKeyframe(m_curFrame);
    m_systemStatus = Status::Process_Second_Frame;
    return Result::Success;
}

System::Result System::processSecondFrame() {
    bool ok = false;
    timed("klt", [&] {
        ok = algorithm::computeOpticalFlowSparse(m_ctx, m_refFrame, m_curFrame, m_config.m_patchSizeOpticalFlow,
                                                 m_config.m_disparityThreshold);
    });
    if (!ok) return Result::Failed;
    const uint32_t thresholdCorrespondingPoints = m_config.m_minDetectedPointsSuccessInitialization * 0.5;
    std::array<double, 9> E{};
    timed("essential", [&] {
        ok = algorithm::computeEssentialMatrix(m_ctx, m_refFrame, m_curFrame, 1.0, thresholdCorrespondingPoints, E,
                                               m_config.m_ransacSeed);
    });
    if (!ok) return Result::Failed;
    timed("two_view", [&] {
        ok = initializeTwoView(m_ctx, m_refFrame, m_curFrame, E, m_config.m_initMapScaleFactor, m_config.m_cellPixelSize).ok;
    });
    if (!ok) return Result::Failed;
    runBA({m_refFrame, m_curFrame}, [&] { m_bundler.twoViewBA(m_refFrame, m_curFrame, 2.0); });
    m_curFrame->setKeyframe();
    m_activeKeyframe = m_curFrame;
    std::vector<double> depths;
    algorithm::normalizedDepthCamera(m_curFrame, depths);
    const double medianDepth = algorithm::computeMedian(depths);
    const double minDepth = *std::min_element(depths.begin(), depths.end());
    m_featureSelector.setExistingFeatures(m_curFrame->m_features);
    select(m_curFrame);
    m_depthEstimator.addKeyframe(m_curFrame, medianDepth, 0.5 * minDepth);
    m_map.addKeyframe(m_curFrame);
    m_systemStatus = Status::Procese_New_Frame;
    return Result::Success;
}

System::Result System::processNewFrame() {
    m_curFrame->m_absPose = poseCompose(m_predictionRelativePose, m_refFrame->m_absPose);
    timed("align", [&] { m_alignment.align(m_refFrame, m_curFrame); });
    std::vector<std::pair<std::shared_ptr<Frame>, int32_t>> overlapKeyFrames;
    timed("reproject", [&] { m_map.reprojectMap(m_refFrame, m_curFrame, overlapKeyFrames); });
    timed("candidates", [&] { m_map.addCandidateToFrame(m_curFrame); });
    if (!computeTrackingQuality(m_curFrame, m_refFrame->numberObservationWithPoints())) {
        m_curFrame->m_absPose = m_refFrame->m_absPose;
        return Result::Success;
    }
    std::vector<double> depths;
    algorithm::normalizedDepthCamera(m_curFrame, depths);
    const double depthMean = algorithm::computeMedian(depths);
    const double depthMin = *std::min_element(depths.begin(), depths.end());
    if (needKeyframe()) {
        timed("depth", [&] { m_depthEstimator.addFrame(m_curFrame); });
        return Result::Success;
    }
    m_curFrame->setKeyframe();
    m_map.addKeyframe(m_curFrame);
    m_activeKeyframe = m_curFrame;
    runBA(m_map.m_keyFrames, [&] { m_bundler.localBA(m_map.m_keyFrames, 2.0); });
    m_featureSelector.setExistingFeatures(m_curFrame->m_features);
    select(m_curFrame);
    m_depthEstimator.addKeyframe(m_curFrame, depthMean, depthMin * 0.5);
    if (m_map.sizeKeyframes() > m_config.m_maxKeyframes) {  // :436-442
        std::shared_ptr<Frame> furthestFrame;
        m_map.getFurthestKeyframe(m_curFrame->cameraInWorld(), furthestFrame);
        m_depthEstimator.removeKeyframe(furthestFrame);
        m_map.removeFrame(furthestFrame);
    }
    return Result::Keyframe;
}

System::Result System::relocalizeFrame(std::shared_ptr<Frame>& closestKeyframe) {
    if (closestKeyframe == nullptr) return Result::Failed;
    if (!closestKeyframe->m_lastKeyframe)  // (the reference dereferences the null pointer in ImageAlignment::align)
        throw Error(SVO_ERR_ARG, "svo: relocalisation against a keyframe without a last keyframe");
    timed("align", [&] { m_alignment.align(closestKeyframe, m_curFrame); });
    return Result::Success;
}

bool System::computeTrackingQuality(const std::shared_ptr<Frame>& frame, uint32_t refFrameNumberObservations) const {
    const int32_t curNumberObservations = (int32_t)frame->numberObservation();
    if (frame->numberObservation() < 50) return false;
    return !((int32_t)refFrameNumberObservations - curNumberObservations > 40);
}

bool System::needKeyframe() const {  // (the other quantities of :485-501 only feed the reference's log)
    return m_curFrame->m_id - m_curFrame->m_lastKeyframe->m_id < 3;
}

System::Summary System::reportSummary() const {
    Summary s;
    std::vector<const Frame*> frames;
    for (const auto& k : m_map.m_keyFrames) frames.push_back(k.get());
    for (const auto* fr : {m_refFrame.get(), m_curFrame.get()})
        if (fr && std::find(frames.begin(), frames.end(), fr) == frames.end()) frames.push_back(fr);
    std::vector<const Point*> points;
    for (const auto* fr : frames) {
        s.features += fr->numberObservation();
        for (const auto& f : fr->m_features)
            if (f->m_point && std::find(points.begin(), points.end(), f->m_point.get()) == points.end())
                points.push_back(f->m_point.get());
    }
    s.frames = frames.size();
    s.points = points.size();
    s.filters = m_depthEstimator.numberFilters();
    s.candidates = m_map.m_candidates.size();
    s.keyframes = m_map.sizeKeyframes();
    return s;
}

// ------------------------------------------------------------------ trajectory / feature dump
namespace utils {
void writeInFile(const Pose& refAbsPose, std::ostream& w) {
    double m[12];
    check(svo_pose_matrix3x4_inverse(refAbsPose.data(), m));
    w << std::setprecision(6);
    for (int i = 0; i < 12; ++i) w << (i ? " " : "") << m[i];
    w << std::endl;
}

void writeAllInfoFile(const Frame& ref, const Frame& cur, std::ostream& w) {
    for (std::size_t i = 0; i < ref.numberObservation(); i++) {
        const Vec2& r = ref.m_features[i]->m_pixelPosition;
        const Vec2& c = cur.m_features[i]->m_pixelPosition;
        const Vec3& p = ref.m_features[i]->m_point->m_position;
        w << std::setprecision(6) << r[0] << " " << r[1] << " " << c[0] << " " << c[1] << " " << p[0] << " " << p[1]
          << " " << p[2] << std::endl;
    }
}

void writeFeaturesInfoFile(const Frame& ref, const Frame& cur, std::ostream& w) {
    for (std::size_t i = 0; i < ref.numberObservation(); i++) {
        const Vec2& r = ref.m_features[i]->m_pixelPosition;
        const Vec2& c = cur.m_features[i]->m_pixelPosition;
        w << std::setprecision(6) << r[0] << " " << r[1] << " " << c[0] << " " << c[1] << std::endl;
    }
}
}  // namespace utils

}  // namespace svo_amd
