// svo_host_check.cpp — drives the C++ class-surface mirror (host/svo.hpp, libsvo_host.so) from the tests.
//   svo_host_check io              poses on stdin (7 numbers a line, Sophus params) -> utils::writeInFile lines
//   svo_host_check fs W H CELL THR NUM BUCKET IMAGE.raw [EX EY]...
//                                  FeatureSelection::gradientMagnitudeWithSSC on a raw 8-bit image (GPU);
//                                  existing features (EX, EY) marked first; prints "x y response" per feature
//   svo_host_check fv W H CELL THR IMAGE.raw    gradientMagnitudeByValue (bucketing)
//   svo_host_check ba N DATA.bin   BundleAdjustment::optimizePose twice on one object (GPU); DATA.bin:
//                                  pose[7], then per feature bearing[3] point[3] has_point (as a double);
//                                  prints "err status qx qy qz qw tx ty tz" per call
//   svo_host_check depth DATA.bin KF.raw CUR.raw   DepthEstimator addKeyframe + updateFilters (GPU);
//                                  DATA.bin: fx fy cx cy W H, kf pose[7], cur pose[7], depth_mean, depth_min,
//                                  n, then n x (px[2] bearing[3]) as doubles; prints "filters M", then one
//                                  "cand X Y Z" line per candidate
//   svo_host_check map DATA.bin REF.raw KF.raw CUR.raw   Map::reprojectMap + addCandidateToFrame (GPU);
//                                  DATA.bin (doubles): fx fy cx cy W H cell, ref/kf/cur pose[7], n_ref n_kf
//                                  n_points n_cand n_cells, feat_px[2n], feat_point[n], point_pos[3p],
//                                  point_type[p], point_succ[p], cand_feat[c], cand_pos[3c], cell_order;
//                                  prints "counts matches trials", then "px X Y" per new cur feature;
//                                  an optional REPS argument also times REPS more runs on fresh object
//                                  graphs ("ms T": reprojectMap + addCandidateToFrame, average)
//   svo_host_check align DATA.bin REF.raw KF.raw CUR.raw PATCH MINL MAXL MEDIAN
//                                  ImageAlignment::align (GPU) twice on one object from the same initial
//                                  cur pose (the second call reuses the object's batch); DATA.bin (doubles):
//                                  fx fy cx cy W H, ref/kf/cur pose[7], n_ref n_kf, then per feature
//                                  px[2] bearing[3] point[3] has_point; prints "err status pose[7]" per call
//   svo_host_check init DATA.bin   initializeTwoView (GPU); DATA.bin (doubles): fx fy cx cy W H, ref pose[7], E[9]
//                                  row-major, map_scale, cell, n, then n x (ref px[2] cur px[2]); prints
//                                  "init ok winner c0 c1 c2 c3 n_points median", "pose" + cur pose[7], then per
//                                  feature left "pt refx refy curx cury X Y Z" (no X Y Z when the call failed),
//                                  then "tri X Y Z" per feature: algorithm::triangulate3DWorldPoints on the result
//   svo_host_check wba DATA.bin    BundleAdjustment::twoViewBA / localBA (GPU; `ba` is optimizePose above); DATA.bin
//                                  (doubles): fx fy cx cy W H, reprojection error, local (0: twoViewBA of frames 0
//                                  and 1, 1: localBA), n_key, n_frames, n_frames x pose[7], n_points, n_points x X[3],
//                                  n_edges, n_edges x (frame point px py): one Feature per edge, appended to its frame
//                                  and to its point in edge order, the first n_key frames the keyframes; prints with
//                                  %a "chi init final removed", per frame "pose p[7]" and "left n", per point
//                                  "pt X Y Z type observations"
//   svo_host_check klt IMAGES.raw W H PX.bin N WIN THR   algorithm::computeOpticalFlowSparse (GPU); IMAGES.raw: the
//                                  ref then the cur image (W x H bytes each); PX.bin: N x px[2] doubles, the ref
//                                  frame's features; prints "klt result n_ref n_cur", then with %a "ref x y" per
//                                  feature left in the ref frame and "cur x y" per feature of the cur frame
//   svo_host_check system DATA.bin IMAGES.raw   System::addImage over a sequence (GPU); DATA.bin (doubles): fx fy cx cy
//                                  W H, cell, desired points, min points, disparity threshold, map scale, ransac
//                                  seed, max keyframes, patch (optical flow), patch (alignment), min level, max
//                                  level, gradient threshold, median mode, n_frames, relocalise (1: the status is set
//                                  to relocalisation before the last frame), n_cells, the map's cell order, then
//                                  optionally d0 .. d4 (the lens; the frames are then raw images), then optionally
//                                  pixel_format (SVO_PIXEL_*) and gray16_shift (absent: 8-bit grey frames);
//                                  IMAGES.raw: the frames, packed, W x H pixels of that format each; prints per frame "frame k result status
//                                  keyframe n_obs n_obs_points seeds candidates keyframes", "pose" + the cur pose[7]
//                                  with %a, "removed" + frame:index of the features the BA removed (frame ids
//                                  relative to the first), "time" + step=seconds, and last the trajectory lines; an
//                                  optional PASSES argument repeats the whole run on a fresh System (timing)
//   svo_host_check undistort_points DATA.bin   PinholeCamera::rawPixel / undistortedPixel (host only); DATA.bin (doubles):
//                                  fx fy cx cy W H d0 .. d4 n, then n x p[2]; prints with %a per point "pt" + rawPixel(p)
//                                  + undistortedPixel(rawPixel(p))
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "svo.hpp"

using namespace svo_amd;

static std::vector<uint8_t> read_raw(const char* path, size_t n) {
    std::ifstream f(path, std::ios::binary);
    std::vector<uint8_t> v((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (v.size() != n) throw std::runtime_error("image size mismatch");
    return v;
}

int main(int argc, char** argv) {
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if (mode == "io") {
            Pose p;
            while (std::cin >> p[0] >> p[1] >> p[2] >> p[3] >> p[4] >> p[5] >> p[6]) utils::writeInFile(p, std::cout);
            return 0;
        }
        if ((mode == "fs" && argc >= 9) || (mode == "fv" && argc >= 7)) {
            const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), cell = std::atoi(argv[4]), thr = std::atoi(argv[5]);
            const char* img_path = mode == "fs" ? argv[8] : argv[6];
            const std::vector<uint8_t> img = read_raw(img_path, (size_t)w * h);
            Context ctx(0);
            auto cam = std::make_shared<PinholeCamera>(PinholeCamera{w, h, 300.0, 300.0, w / 2.0, h / 2.0});
            auto frame = std::make_shared<Frame>(ctx, cam, img.data(), 1);
            FeatureSelection sel(ctx, w, h, cell);
            std::vector<std::shared_ptr<Feature>> existing;
            if (mode == "fs")
                for (int i = 9; i + 1 < argc; i += 2)
                    existing.push_back(std::make_shared<Feature>(frame.get(), Vec2{std::atof(argv[i]), std::atof(argv[i + 1])}));
            auto run = [&]() {
                frame->m_features.clear();
                sel.resetGridOccupancy();
                sel.setExistingFeatures(existing);
                if (mode == "fs") sel.gradientMagnitudeWithSSC(frame, thr, std::atoi(argv[6]), std::atoi(argv[7]) != 0);
                else sel.gradientMagnitudeByValue(frame, thr, true);
            };
            run();
            for (const auto& f : frame->m_features)
                std::printf("%.17g %.17g %.17g\n", f->m_pixelPosition[0], f->m_pixelPosition[1], f->m_gradientMagnitude);
            // SVO_CHECK_REPS=n: time n more calls (selection only; the grid reset / existing features are
            // inside the loop but cost nanoseconds) and report the average on stderr
            const char* reps_env = std::getenv("SVO_CHECK_REPS");
            const int reps = reps_env ? std::atoi(reps_env) : 0;
            if (reps > 0) {
                const auto t0 = std::chrono::steady_clock::now();
                for (int r = 0; r < reps; ++r) run();
                const auto t1 = std::chrono::steady_clock::now();
                std::fprintf(stderr, "ms %.6f\n", std::chrono::duration<double, std::milli>(t1 - t0).count() / reps);
            }
            return 0;
        }
        if (mode == "ba" && argc >= 4) {
            const int n = std::atoi(argv[2]);
            std::ifstream f(argv[3], std::ios::binary);
            std::vector<double> d(7 + 7 * (size_t)n);
            f.read(reinterpret_cast<char*>(d.data()), (std::streamsize)(d.size() * sizeof(double)));
            if (!f) throw std::runtime_error("short BA data file");
            Context ctx(0);
            auto cam = std::make_shared<PinholeCamera>(PinholeCamera{64, 64, 300.0, 300.0, 32.0, 32.0});
            std::vector<uint8_t> img(64 * 64, 0);
            auto frame = std::make_shared<Frame>(ctx, cam, img.data(), 1);
            for (int i = 0; i < 7; ++i) frame->m_absPose[i] = d[i];
            for (int k = 0; k < n; ++k) {
                const double* r = &d[7 + 7 * (size_t)k];
                auto feat = std::make_shared<Feature>(frame.get(), Vec2{0.0, 0.0});
                feat->m_bearingVec = {r[0], r[1], r[2]};
                if (r[6] != 0.0) feat->m_point = std::make_shared<Point>(Point{{r[3], r[4], r[5]}});
                frame->m_features.push_back(feat);
            }
            BundleAdjustment ba(ctx, cam, 0, 6);
            for (int call = 0; call < 2; ++call) {
                const double e = ba.optimizePose(frame);
                std::printf("%.17g %d", e, ba.lastStatus());
                for (double v : frame->m_absPose) std::printf(" %.17g", v);
                std::printf("\n");
            }
            return 0;
        }
        if (mode == "depth" && argc >= 5) {
            std::ifstream f(argv[2], std::ios::binary);
            std::vector<double> hdr(6 + 7 + 7 + 3);
            f.read(reinterpret_cast<char*>(hdr.data()), (std::streamsize)(hdr.size() * sizeof(double)));
            const int w = (int)hdr[4], h = (int)hdr[5], n = (int)hdr[22];
            std::vector<double> d(5 * (size_t)n);
            f.read(reinterpret_cast<char*>(d.data()), (std::streamsize)(d.size() * sizeof(double)));
            if (!f) throw std::runtime_error("short depth data file");
            const std::vector<uint8_t> kimg = read_raw(argv[3], (size_t)w * h), cimg = read_raw(argv[4], (size_t)w * h);
            Context ctx(0);
            auto cam = std::make_shared<PinholeCamera>(PinholeCamera{w, h, hdr[0], hdr[1], hdr[2], hdr[3]});
            auto kf = std::make_shared<Frame>(ctx, cam, kimg.data(), 1);
            auto cur = std::make_shared<Frame>(ctx, cam, cimg.data(), 1);
            for (int i = 0; i < 7; ++i) {
                kf->m_absPose[i] = hdr[6 + i];
                cur->m_absPose[i] = hdr[13 + i];
            }
            for (int k = 0; k < n; ++k) {
                const double* r = &d[5 * (size_t)k];
                auto feat = std::make_shared<Feature>(kf.get(), Vec2{r[0], r[1]});
                feat->m_bearingVec = {r[2], r[3], r[4]};
                kf->m_features.push_back(feat);
            }
            DepthEstimator de(ctx);
            de.addKeyframe(kf, hdr[20], hdr[21]);
            const auto cands = de.updateFilters(cur);
            std::printf("filters %zu\n", de.numberFilters());
            for (const auto& c : cands)
                std::printf("cand %.17g %.17g %.17g\n", c.second->m_position[0], c.second->m_position[1], c.second->m_position[2]);
            return 0;
        }
        if (mode == "init" && argc >= 3) {
            std::ifstream f(argv[2], std::ios::binary);
            f.seekg(0, std::ios::end);
            const size_t bytes = (size_t)f.tellg();
            f.seekg(0);
            std::vector<double> v(bytes / sizeof(double));
            f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)bytes);
            size_t q = 0;
            auto take = [&]() { return v.at(q++); };
            const double fx = take(), fy = take(), cx = take(), cy = take();
            const int w = (int)take(), h = (int)take();
            Pose refPose;
            for (double& x : refPose) x = take();
            std::array<double, 9> E;
            for (double& x : E) x = take();
            const double mapScale = take();
            const int cell = (int)take(), n = (int)take();
            Context ctx(0);
            auto cam = std::make_shared<PinholeCamera>(PinholeCamera{w, h, fx, fy, cx, cy});
            const std::vector<uint8_t> img((size_t)w * h, 0);
            auto ref = std::make_shared<Frame>(ctx, cam, img.data(), 1);
            auto cur = std::make_shared<Frame>(ctx, cam, img.data(), 1);
            ref->m_absPose = refPose;
            for (int i = 0; i < n; ++i) {
                const double rx = take(), ry = take(), ux = take(), uy = take();
                ref->m_features.push_back(std::make_shared<Feature>(ref.get(), Vec2{rx, ry}));
                cur->m_features.push_back(std::make_shared<Feature>(cur.get(), Vec2{ux, uy}));
            }
            const TwoViewResult r = initializeTwoView(ctx, ref, cur, E, mapScale, cell);
            std::printf("init %d %d %d %d %d %d %zu %.17g\n", r.ok ? 1 : 0, r.winner, r.counts[0], r.counts[1], r.counts[2],
                        r.counts[3], r.numPoints, r.medianDepth);
            std::printf("pose");
            for (double x : cur->m_absPose) std::printf(" %.17g", x);
            std::printf("\n");
            for (size_t i = 0; i < ref->numberObservation(); ++i) {
                const auto& fr = ref->m_features[i];
                const auto& fc = cur->m_features[i];
                if (r.ok && (fr->m_point != fc->m_point || fr->m_point->m_features.size() != 2))
                    throw std::runtime_error("ref / cur features do not share their point");
                std::printf("pt %.17g %.17g %.17g %.17g", fr->m_pixelPosition[0], fr->m_pixelPosition[1],
                            fc->m_pixelPosition[0], fc->m_pixelPosition[1]);
                if (fr->m_point)
                    std::printf(" %.17g %.17g %.17g", fr->m_point->m_position[0], fr->m_point->m_position[1],
                                fr->m_point->m_position[2]);
                std::printf("\n");
            }
            if (r.ok) {  // triangulate3DWorldPoints on the initialised frames
                std::vector<Vec3> tri;
                algorithm::triangulate3DWorldPoints(ctx, ref, cur, tri);
                for (const Vec3& x : tri) std::printf("tri %.17g %.17g %.17g\n", x[0], x[1], x[2]);
            }
            return 0;
        }
        if (mode == "klt" && argc >= 9) {
            const int w = std::atoi(argv[3]), h = std::atoi(argv[4]), n = std::atoi(argv[6]), win = std::atoi(argv[7]);
            const double thr = std::atof(argv[8]);
            const std::vector<uint8_t> imgs = read_raw(argv[2], 2 * (size_t)w * h);
            std::vector<double> px(2 * (size_t)n);
            std::ifstream f(argv[5], std::ios::binary);
            f.read(reinterpret_cast<char*>(px.data()), (std::streamsize)(px.size() * sizeof(double)));
            if (!f) throw std::runtime_error("short pixel file");
            Context ctx(0);
            auto cam = std::make_shared<PinholeCamera>(PinholeCamera{w, h, 150.0, 150.0, w / 2.0, h / 2.0});
            auto ref = std::make_shared<Frame>(ctx, cam, imgs.data(), 4);
            auto cur = std::make_shared<Frame>(ctx, cam, imgs.data() + (size_t)w * h, 4);
            for (int i = 0; i < n; ++i)
                ref->m_features.push_back(std::make_shared<Feature>(ref.get(), Vec2{px[2 * i], px[2 * i + 1]}));
            const bool ok = algorithm::computeOpticalFlowSparse(ctx, ref, cur, (uint32_t)win, thr);
            std::printf("klt %d %zu %zu\n", ok ? 1 : 0, ref->numberObservation(), cur->numberObservation());
            for (const auto& ft : ref->m_features) std::printf("ref %a %a\n", ft->m_pixelPosition[0], ft->m_pixelPosition[1]);
            for (const auto& ft : cur->m_features) {
                if (ft->m_frame != cur.get() || ft->m_gradientMagnitude != 0.0 || ft->m_gradientOrientation != 0.0 || ft->m_point)
                    throw std::runtime_error("cur feature is not Feature(cur, px, 0.0, 0.0, 0)");
                std::printf("cur %a %a\n", ft->m_pixelPosition[0], ft->m_pixelPosition[1]);
            }
            return 0;
        }
        if (mode == "essential" && argc >= 3) {
            // DATA.bin (doubles): fx fy cx cy w h reproError threshold seed n, then n x (ref.x ref.y cur.x cur.y)
            std::ifstream f(argv[2], std::ios::binary);
            f.seekg(0, std::ios::end);
            const size_t bytes = (size_t)f.tellg();
            f.seekg(0);
            std::vector<double> v(bytes / sizeof(double));
            f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)bytes);
            size_t q = 0;
            auto take = [&]() { return v.at(q++); };
            const double fx = take(), fy = take(), cx = take(), cy = take();
            const int w = (int)take(), h = (int)take();
            const double reproError = take();
            const uint32_t threshold = (uint32_t)take();
            const uint64_t seed = (uint64_t)take();
            const int n = (int)take();
            Context ctx(0);
            auto cam = std::make_shared<PinholeCamera>(PinholeCamera{w, h, fx, fy, cx, cy});
            const std::vector<uint8_t> img((size_t)w * h, 0);
            auto ref = std::make_shared<Frame>(ctx, cam, img.data(), 1);
            auto cur = std::make_shared<Frame>(ctx, cam, img.data(), 1);
            for (int i = 0; i < n; ++i) {
                const double rx = take(), ry = take(), ux = take(), uy = take();
                ref->m_features.push_back(std::make_shared<Feature>(ref.get(), Vec2{rx, ry}));
                cur->m_features.push_back(std::make_shared<Feature>(cur.get(), Vec2{ux, uy}));
            }
            std::array<double, 9> E{};
            const bool ok = algorithm::computeEssentialMatrix(ctx, ref, cur, reproError, threshold, E, seed);
            std::printf("essential %d %zu %zu\n", ok ? 1 : 0, ref->numberObservation(), cur->numberObservation());
            std::printf("E");
            for (double x : E) std::printf(" %a", x);
            std::printf("\n");
            for (const auto& ft : ref->m_features) std::printf("ref %a %a\n", ft->m_pixelPosition[0], ft->m_pixelPosition[1]);
            for (const auto& ft : cur->m_features) std::printf("cur %a %a\n", ft->m_pixelPosition[0], ft->m_pixelPosition[1]);
            return 0;
        }
        if (mode == "wba" && argc >= 3) {
            std::ifstream f(argv[2], std::ios::binary);
            f.seekg(0, std::ios::end);
            const size_t bytes = (size_t)f.tellg();
            f.seekg(0);
            std::vector<double> v(bytes / sizeof(double));
            f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)bytes);
            size_t q = 0;
            auto take = [&]() { return v.at(q++); };
            const double fx = take(), fy = take(), cx = take(), cy = take();
            const int w = (int)take(), h = (int)take();
            const double reproj = take();
            const bool local = take() != 0.0;
            const int nKey = (int)take(), nFrames = (int)take();
            Context ctx(0);
            auto cam = std::make_shared<PinholeCamera>(PinholeCamera{w, h, fx, fy, cx, cy});
            const std::vector<uint8_t> img((size_t)w * h, 0);
            std::vector<std::shared_ptr<Frame>> frames;
            for (int i = 0; i < nFrames; ++i) {
                frames.push_back(std::make_shared<Frame>(ctx, cam, img.data(), 1));
                for (double& x : frames.back()->m_absPose) x = take();
            }
            std::vector<std::shared_ptr<Point>> points;
            const int nPoints = (int)take();
            for (int j = 0; j < nPoints; ++j) {
                const double x = take(), y = take(), z = take();
                points.push_back(std::make_shared<Point>(Point{{x, y, z}}));
            }
            const int nEdges = (int)take();
            for (int k = 0; k < nEdges; ++k) {
                const int i = (int)take(), j = (int)take();
                const double px = take(), py = take();
                auto feature = std::make_shared<Feature>(frames.at(i).get(), Vec2{px, py});
                feature->m_point = points.at(j);
                points[j]->m_features.push_back(feature);
                frames[i]->m_features.push_back(feature);
            }
            BundleAdjustment bundler(ctx, cam, 0, 6);
            std::vector<std::shared_ptr<Frame>> keyFrames(frames.begin(), frames.begin() + nKey);
            const BundleAdjustment::WindowResult r =
                local ? bundler.localBA(keyFrames, reproj) : bundler.twoViewBA(frames.at(0), frames.at(1), reproj);
            std::printf("chi %a %a %u\n", r.initError, r.finalError, r.removed);
            for (const auto& fr : frames) {
                std::printf("pose");
                for (double x : fr->m_absPose) std::printf(" %a", x);
                std::printf("\nleft %zu\n", fr->numberObservation());
            }
            for (const auto& p : points)
                std::printf("pt %a %a %a %u %zu\n", p->m_position[0], p->m_position[1], p->m_position[2],
                            (unsigned)p->m_type, p->numberObservation());
            return 0;
        }
        if (mode == "align" && argc >= 10) {
            std::ifstream f(argv[2], std::ios::binary);
            f.seekg(0, std::ios::end);
            const size_t bytes = (size_t)f.tellg();
            f.seekg(0);
            std::vector<double> v(bytes / sizeof(double));
            f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)bytes);
            size_t q = 0;
            auto take = [&]() { return v.at(q++); };
            const double fx = take(), fy = take(), cx = take(), cy = take();
            const int w = (int)take(), h = (int)take();
            Pose poses[3];
            for (auto& p : poses)
                for (double& x : p) x = take();
            const int nref = (int)take(), nkf = (int)take();
            const int patch = std::atoi(argv[6]), minl = std::atoi(argv[7]), maxl = std::atoi(argv[8]);
            const int median = std::atoi(argv[9]);
            const std::vector<uint8_t> rimg = read_raw(argv[3], (size_t)w * h), kimg = read_raw(argv[4], (size_t)w * h),
                                       cimg = read_raw(argv[5], (size_t)w * h);
            Context ctx(0);
            auto cam = std::make_shared<PinholeCamera>(PinholeCamera{w, h, fx, fy, cx, cy});
            auto kf = std::make_shared<Frame>(ctx, cam, kimg.data(), maxl + 1);
            auto ref = std::make_shared<Frame>(ctx, cam, rimg.data(), maxl + 1, kf);
            auto cur = std::make_shared<Frame>(ctx, cam, cimg.data(), maxl + 1, kf);
            ref->m_absPose = poses[0];
            kf->m_absPose = poses[1];
            for (int i = 0; i < nref + nkf; ++i) {
                const double ux = take(), uy = take();
                auto feat = std::make_shared<Feature>(i < nref ? ref.get() : kf.get(), Vec2{ux, uy});
                feat->m_bearingVec = {take(), take(), take()};
                const Vec3 pos{take(), take(), take()};
                if (take() != 0.0) feat->m_point = std::make_shared<Point>(Point{pos});
                (i < nref ? ref : kf)->m_features.push_back(feat);
            }
            ImageAlignment align(ctx, (uint32_t)patch, minl, maxl, 6, median);
            for (int call = 0; call < 2; ++call) {
                cur->m_absPose = poses[2];
                const double e = align.align(ref, cur);
                std::printf("%.17g %d", e, align.lastStatus());
                for (double x : cur->m_absPose) std::printf(" %.17g", x);
                std::printf("\n");
            }
            // REPS > 0: the per-frame latency of align() as src/system.cpp:313 pays it (median of REPS calls)
            const int reps = argc >= 11 ? std::atoi(argv[10]) : 0;
            if (reps > 0) {
                std::vector<double> ms;
                for (int i = 0; i < reps; ++i) {
                    cur->m_absPose = poses[2];
                    const auto t0 = std::chrono::steady_clock::now();
                    align.align(ref, cur);
                    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
                }
                std::sort(ms.begin(), ms.end());
                std::printf("ms %.6f\n", ms[ms.size() / 2]);
            }
            return 0;
        }
        if (mode == "map" && argc >= 6) {
            std::ifstream f(argv[2], std::ios::binary);
            f.seekg(0, std::ios::end);
            const size_t bytes = (size_t)f.tellg();
            f.seekg(0);
            std::vector<double> v(bytes / sizeof(double));
            f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)bytes);
            size_t q = 0;
            auto take = [&]() { return v.at(q++); };
            const double fx = take(), fy = take(), cx = take(), cy = take();
            const int w = (int)take(), h = (int)take(), cell = (int)take();
            Pose poses[3];
            for (auto& p : poses)
                for (double& x : p) x = take();
            const int nref = (int)take(), nkf = (int)take(), npt = (int)take(), nc = (int)take(), ncells = (int)take();
            const int nf = nref + nkf;
            std::vector<Vec2> px(nf);
            for (auto& p : px) p = {take(), take()};
            std::vector<int> fpt(nf);
            for (int& i : fpt) i = (int)take();
            std::vector<Vec3> ppos(npt);
            for (auto& p : ppos) p = {take(), take(), take()};
            std::vector<uint32_t> ptype(npt), psucc(npt);
            for (auto& t : ptype) t = (uint32_t)take();
            for (auto& t : psucc) t = (uint32_t)take();
            std::vector<int> cf(nc);
            for (int& i : cf) i = (int)take();
            std::vector<Vec3> cpos(nc);
            for (auto& p : cpos) p = {take(), take(), take()};
            std::vector<int32_t> order(ncells);
            for (int32_t& o : order) o = (int32_t)take();
            const std::vector<uint8_t> rimg = read_raw(argv[3], (size_t)w * h), kimg = read_raw(argv[4], (size_t)w * h),
                                       cimg = read_raw(argv[5], (size_t)w * h);
            const int reps = argc >= 7 ? std::atoi(argv[6]) : 0;  // > 0: time reprojectMap + addCandidateToFrame
            const bool twice = argc >= 8 && std::string(argv[7]) == "twice";  // then a second addCandidateToFrame
            Context ctx(0);
            auto cam = std::make_shared<PinholeCamera>(PinholeCamera{w, h, fx, fy, cx, cy});
            double total_ms = 0.0;
            for (int rep = 0; rep <= reps; ++rep) {
                // a fresh object graph per run (the calls mutate the map, the points and the cur frame)
                auto kf = std::make_shared<Frame>(ctx, cam, kimg.data(), 1);
                auto ref = std::make_shared<Frame>(ctx, cam, rimg.data(), 1, kf);
                auto cur = std::make_shared<Frame>(ctx, cam, cimg.data(), 1, kf);
                ref->m_absPose = poses[0];
                kf->m_absPose = poses[1];
                cur->m_absPose = poses[2];
                std::vector<std::shared_ptr<Point>> pts(npt);
                for (int i = 0; i < npt; ++i) {
                    pts[i] = std::make_shared<Point>(Point{ppos[i]});
                    pts[i]->m_type = (Point::PointType)ptype[i];
                    pts[i]->m_succeededProjection = psucc[i];
                }
                std::vector<std::shared_ptr<Feature>> feats(nf);
                for (int i = 0; i < nf; ++i) {
                    feats[i] = std::make_shared<Feature>(i < nref ? ref.get() : kf.get(), px[i]);
                    if (fpt[i] >= 0) feats[i]->m_point = pts[fpt[i]];
                    (i < nref ? ref : kf)->m_features.push_back(feats[i]);
                }
                Map map(ctx, cam, cell);
                for (int i = 0; i < nc; ++i) map.addNewCandidate(feats[cf[i]], std::make_shared<Point>(Point{cpos[i]}));
                map.setCellOrder(order);
                std::vector<std::pair<std::shared_ptr<Frame>, int32_t>> overlap;
                (void)svo_ctx_synchronize(ctx.get());
                const auto t0 = std::chrono::steady_clock::now();
                map.reprojectMap(ref, cur, overlap);
                map.addCandidateToFrame(cur);
                const auto t1 = std::chrono::steady_clock::now();
                if (rep > 0) total_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
                if (rep == 0) {
                    std::printf("counts %u %u\n", map.m_matches, map.m_trials);
                    for (const auto& ft : cur->m_features)
                        std::printf("px %.17g %.17g\n", ft->m_pixelPosition[0], ft->m_pixelPosition[1]);
                    if (twice) {  // a second frame (cur moved 5 cm along x): only unmatched candidates remain
                        std::printf("candidates %zu\n", map.m_candidates.size());
                        auto cur2 = std::make_shared<Frame>(ctx, cam, cimg.data(), 1, kf);
                        cur2->m_absPose = poses[2];
                        cur2->m_absPose[4] += 0.05;
                        map.addCandidateToFrame(cur2);
                        std::printf("candidates %zu\n", map.m_candidates.size());
                        for (const auto& ft : cur2->m_features)
                            std::printf("px2 %.17g %.17g\n", ft->m_pixelPosition[0], ft->m_pixelPosition[1]);
                    }
                }
            }
            if (reps > 0) std::printf("ms %.6f\n", total_ms / reps);
            return 0;
        }
        if (mode == "system" && argc >= 4) {
            std::ifstream f(argv[2], std::ios::binary);
            std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            const double* d = reinterpret_cast<const double*>(raw.data());
            const size_t nd = raw.size() / sizeof(double);
            if (nd < 22) throw std::runtime_error("system: DATA.bin too short");
            Config c;
            c.m_fx = d[0]; c.m_fy = d[1]; c.m_cx = d[2]; c.m_cy = d[3];
            c.m_imgWidth = (int32_t)d[4]; c.m_imgHeight = (int32_t)d[5];
            c.m_cellPixelSize = (int32_t)d[6];
            c.m_desiredDetectedPointsForInitialization = (uint32_t)d[7];
            c.m_minDetectedPointsSuccessInitialization = (uint32_t)d[8];
            c.m_disparityThreshold = d[9];
            c.m_initMapScaleFactor = d[10];
            c.m_ransacSeed = (uint64_t)d[11];
            c.m_maxKeyframes = (size_t)d[12];
            c.m_patchSizeOpticalFlow = (uint32_t)d[13];
            c.m_patchSizeImageAlignment = (uint32_t)d[14];
            c.m_minLevelImagePyramid = (int32_t)d[15];
            c.m_maxLevelImagePyramid = (int32_t)d[16];
            c.m_thresholdGradientMagnitude = (uint32_t)d[17];
            c.m_medianMode = (int32_t)d[18];
            const int nFrames = (int)d[19];
            const bool relocalise = d[20] != 0.0;
            const size_t nCells = (size_t)d[21];
            // the optional tail: d0..d4 (5 values), then pixel_format and gray16_shift (2 values), either or both
            const size_t tail = nd - 22 < nCells ? 1 : nd - 22 - nCells;
            if (tail != 0 && tail != 2 && tail != 5 && tail != 7) throw std::runtime_error("system: DATA.bin size mismatch");
            if (tail >= 5) {
                const double* l = d + 22 + nCells;
                c.m_d0 = l[0]; c.m_d1 = l[1]; c.m_d2 = l[2]; c.m_d3 = l[3]; c.m_d4 = l[4];
            }
            if (tail == 2 || tail == 7) {
                c.m_pixelFormat = (int32_t)d[nd - 2];
                c.m_gray16Shift = (int32_t)d[nd - 1];
            }
            const svo_image_layout packed{c.m_pixelFormat, c.m_gray16Shift, 0, 0};
            int64_t layoutBytes = 0;  // of one packed frame in the Config's pixel format
            if (svo_image_layout_bytes(&packed, c.m_imgWidth, c.m_imgHeight, 1, &layoutBytes) != SVO_OK)
                throw std::runtime_error(std::string("system: ") + svo_last_error());
            std::vector<int32_t> order(nCells);
            for (size_t i = 0; i < nCells; ++i) order[i] = (int32_t)d[22 + i];
            const size_t frameBytes = (size_t)layoutBytes;
            const std::vector<uint8_t> imgs = read_raw(argv[3], frameBytes * (size_t)nFrames);
            const int passes = argc > 4 ? std::atoi(argv[4]) : 1;
            Context ctx(0);
            for (int pass = 0; pass < passes; ++pass) {
                System system(ctx, c);
                if (nCells) system.map().setCellOrder(order);
                system.setInstrument(true);
                std::ostringstream trajectory;
                uint64_t base = 0;
                for (int k = 0; k < nFrames; ++k) {
                    if (relocalise && k == nFrames - 1) system.setStatus(System::Status::Process_Relocalization);
                    const auto t0 = std::chrono::steady_clock::now();
                    system.addImage(imgs.data() + frameBytes * (size_t)k, (uint64_t)k);
                    const double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                    const auto& cur = system.curFrame();
                    if (k == 0) base = cur->m_id;
                    std::printf("frame %d %d %d %d %zu %u %zu %zu %zu\n", k, (int)system.lastResult(), (int)system.status(),
                                cur->isKeyframe() ? 1 : 0, cur->numberObservation(), cur->numberObservationWithPoints(),
                                system.depthEstimator().numberFilters(), system.map().m_candidates.size(),
                                system.map().sizeKeyframes());
                    std::printf("pose");
                    for (double v : cur->m_absPose) std::printf(" %a", v);
                    std::printf("\nremoved");
                    for (const auto& r : system.baRemoved()) std::printf(" %llu:%zu", (unsigned long long)(r.first - base), r.second);
                    std::printf("\ntime total=%.9f", total);
                    for (const auto& t : system.timings()) std::printf(" %s=%.9f", t.first.c_str(), t.second);
                    std::printf("\n");
                    if (system.refFrame()) system.writeInFile(trajectory);
                }
                std::printf("trajectory\n%s", trajectory.str().c_str());
            }
            return 0;
        }
        if (mode == "undistort_points" && argc >= 3) {
            std::ifstream f(argv[2], std::ios::binary);
            std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            const double* d = reinterpret_cast<const double*>(raw.data());
            const size_t nd = raw.size() / sizeof(double);
            if (nd < 12 || nd != 12 + 2 * (size_t)d[11]) throw std::runtime_error("undistort_points: DATA.bin size mismatch");
            const PinholeCamera cam{(int32_t)d[4], (int32_t)d[5], d[0], d[1], d[2], d[3], d[6], d[7], d[8], d[9], d[10]};
            for (size_t i = 0; i < (size_t)d[11]; ++i) {
                const Vec2 r = cam.rawPixel({d[12 + 2 * i], d[13 + 2 * i]}), u = cam.undistortedPixel(r);
                std::printf("pt %a %a %a %a\n", r[0], r[1], u[0], u[1]);
            }
            return 0;
        }
        std::fprintf(stderr, "usage: svo_host_check io | fs W H CELL THR NUM BUCKET IMAGE [EX EY]... | fv W H CELL THR IMAGE | init DATA.bin | essential DATA.bin | wba DATA.bin | system DATA.bin IMAGES.raw [PASSES] | undistort_points DATA.bin\n");
        return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "svo_host_check: %s\n", e.what());
        return 1;
    }
}
