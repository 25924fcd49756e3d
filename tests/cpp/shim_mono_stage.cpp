// shim_mono_stage.cpp -- test driver: uvo_hip::set_mono_pose_stage through the uvo_libraries function surface.  estimate_relative_pose
// (visual_odometry.h:323) runs on the same points with the pose stage at 0 and at 1; after each call the route figures are read from the
// shim's own context (uvo_mono_pose_stats).  The value must survive a rebuilt context, and a value other than 0 / 1 must be refused.
//   usage: shim_mono_stage <input.bin> <output.bin>
//   input : as shim_mono_pose: int32 n, essential_method, homography_method; f64 K[9], essential_threshold, homography_threshold; n x (x1,y1) f32; n x (x2,y2) f32
//   output: three records (stage 0, stage 1, stage 1 after shutdown()): int32 use_essential_out, success, n_inliers, attempts[4]; f64 R[9], t[3]
#include <cstdio>
#include <vector>
#include "uvo_libraries_hip/VO_utility_hip.h"
using namespace uvocv;

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[3]; double cam[11];
    if (fread(hdr, sizeof(int), 3, f) != 3 || fread(cam, sizeof(double), 11, f) != 11) return 2;
    const int n = hdr[0];
    std::vector<Point2f> k1((size_t)n), k2((size_t)n);
    if (fread(static_cast<void*>(k1.data()), sizeof(Point2f), n, f) != (size_t)n || fread(static_cast<void*>(k2.data()), sizeof(Point2f), n, f) != (size_t)n) return 2;
    fclose(f);
    uvo_params mp; uvo_params_default_mono(&mp);
    DISTANCE = mp.DISTANCE; VPF_THRESHOLD = mp.VPF_THRESHOLD; MIN_NUM_INLIERS = mp.MIN_NUM_INLIERS; HOMOGRAPHY_DISTANCE = mp.HOMOGRAPHY_DISTANCE;
    ESSENTIAL_MAX_ITERS = mp.ESSENTIAL_MAX_ITERS; ESSENTIAL_CONFIDENCE = mp.ESSENTIAL_CONFIDENCE;
    HOMOGRAPHY_MAX_ITERS = mp.HOMOGRAPHY_MAX_ITERS; HOMOGRAPHY_CONFIDENCE = mp.HOMOGRAPHY_CONFIDENCE;
    REPROJECTION_TOLERANCE = mp.REPROJECTION_TOLERANCE; MIN_NUM_3DPOINTS = mp.MIN_NUM_3DPOINTS; MIN_NUM_FEATURES = mp.MIN_NUM_FEATURES;
    ESSENTIAL_OUTLIER_METHOD = hdr[1]; HOMOGRAPHY_OUTLIER_METHOD = hdr[2];
    ESSENTIAL_THRESHOLD = cam[9]; HOMOGRAPHY_THRESHOLD = cam[10];
    Mat K(3, 3, CV_64FC1);
    for (int i = 0; i < 9; i++) K.at<double>(i / 3, i % 3) = cam[i];
    try {
        bool refused = false;
        try { uvo_hip::set_mono_pose_stage(2); } catch (const uvo_hip::Error& e) { refused = e.status == UVO_INVALID_ARG; }
        if (!refused) { fprintf(stderr, "set_mono_pose_stage(2) was not refused with UVO_INVALID_ARG\n"); return 3; }
        const bool first = select_estimation_method(k1, k2);
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        for (int pass = 0; pass < 3; pass++) {
            if (pass < 2) uvo_hip::set_mono_pose_stage(pass);
            else uvo_hip::shutdown();                                                        // the next call builds a new context: the value is kept
            use_essential = first;
            Mat R = Mat::eye(3, 3, CV_64FC1), t = Mat::zeros(3, 1, CV_64FC1);
            std::vector<Point2f> in1, in2; std::vector<DMatch> im; bool success = false;
            estimate_relative_pose(k1, k2, K, R, t, in1, in2, im, success);
            int rec[7] = { use_essential ? 1 : 0, success ? 1 : 0, (int)in1.size(), 0, 0, 0, 0 };
            if (uvo_mono_pose_stats(uvo_hip::context(), rec + 3, nullptr, nullptr, nullptr, nullptr) != UVO_OK) return 4;
            fwrite(rec, sizeof(int), 7, o);
            double rt[12];
            for (int i = 0; i < 9; i++) rt[i] = R.at<double>(i / 3, i % 3);
            for (int i = 0; i < 3; i++) rt[9 + i] = t.at<double>(i, 0);
            fwrite(rt, sizeof(double), 12, o);
        }
        fclose(o);
    } catch (const uvo_hip::Error& e) {
        fprintf(stderr, "uvo_hip::Error: %s\n", e.what());
        return 1;
    }
    uvo_hip::shutdown();
    return 0;
}
