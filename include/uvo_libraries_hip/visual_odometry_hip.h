// visual_odometry_hip.h -- the node class of the reference (uvo/include/visual_odometry.h:35-113) without ROS: the same
// callbacks, the same two loops written against the uvo_libraries function surface, one loop iteration per spin_once().
//
// visual_odometry_core keeps what `visual_odometry_node` keeps between iterations (first_img / new_img_available /
// vo_initialized, the previous frame's keypoints and descriptors, the "after stereo match" sets, R / t / SF) and returns what
// the node publishes on /estimated_linear_vel_{mono,stereo}_UVO and /validity_{mono,stereo}_UVO.  The ROS adapter
// (ergo_uvo_amd/ros/UVO_node_hip.cpp, compiled only where roscpp exists) wires the topics to these methods; the tests drive
// it directly (tests/cpp/shim_vo_node.cpp) and compare every published sample with the CPU oracle's state machines.
//
// Execution::operators (the default) runs the loops operator by operator through host Mats, as the reference's node does.
// Execution::fused runs the same iteration as ONE call of the library's camera-frames loop entry (uvo_stereo_step_frames /
// uvo_mono_step_frames, include/uvo_hip.h): get_image, detection, matching and the pose stay on the device, and the node only maps the
// entry's result onto what it publishes.  The reference's quirks (appended init matches, state carried with empty sets after a failed
// gate, the last t_prevCam_currCam published again) live in that entry and are not repeated here.  For recorded sequences the fused
// mode also has a pipelined form: spin_submit() / spin_collect() keep up to set_depth() frames in flight.
// The callbacks also take the compressed message itself (CompressedMessage: the payload and the format string of a
// sensor_msgs/CompressedImage; the node keeps its own copy).  Execution::fused hands it to the compressed loop entries
// (uvo_stereo_step_compressed / uvo_stereo_submit_compressed and the mono twins: the JPEG is decoded on the device, on the entry's lane),
// and no image buffer is kept until the collect.  A payload those entries refuse by kind (PNG, for one) is decoded with
// decode_compressed_image_device and goes through the frames entry instead; that decode works in lane 0's buffers, so with frames in
// flight it is the library's refusal (spin_collect first).  Execution::operators decodes the message to a host Mat as before.
//
// Line references: VO = uvo/include/visual_odometry.h of the reference.
#pragma once
#include <cmath>
#include <deque>
#include <string>
#include <vector>
#include "uvo_libraries_hip/uvo_config.h"
#include "uvo_libraries_hip/image_codec.h"

namespace uvo_hip {

struct Published {
    bool   published = false;          // something went out on the two topics in this iteration
    bool   valid = false;              // std_msgs/Bool on /validity_*_UVO
    double v[3] = {0, 0, 0};           // geometry_msgs/Vector3Stamped.vector on /estimated_linear_vel_*_UVO
    double stamp = 0;                  // header stamp of the frame that produced it
    int    n_kps = 0, n_matches = 0, n_inliers = 0, n_good3d = 0;     // diagnostics (ROS_INFO lines of the reference)
};

enum class Execution { operators, fused };

// a sensor_msgs/CompressedImage as the node keeps it: CompressedImage.data and CompressedImage.format
struct CompressedMessage { std::vector<unsigned char> data; std::string format; };

class visual_odometry_core {
public:
    // VO_NODE: "mono" or "stereo" (rosparam /visual_odometry_node, NODE:23); CAMERA_NAME: rosparam /camera_name (VO:756)
    visual_odometry_core(const std::string& VO_NODE, const ParamTree& params, const std::string& CAMERA_NAME, Execution exec = Execution::operators)
        : mode_(VO_NODE), exec_(exec)
    {
        if (mode_ != "mono" && mode_ != "stereo") throw Error(UVO_INVALID_ARG, "WRONG SELECTION OF VISUAL ODOMETRY NODE - CHOOSE BETWEEN mono AND stereo");   // VO:789
        get_VO_parameters(params);                                                       // VO:757
        if (mode_ == "mono") check_outlier_methods();                                    // an unserved estimator method ends the node here, by name, not at its first estimate
        if (mode_ == "stereo") get_stereo_camera_parameters(params, CAMERA_NAME);        // VO:776
        else get_mono_camera_parameters(params, CAMERA_NAME);                            // VO:787
        R_currCam_prevCam_ = uvocv::Mat::eye(3, 3, uvocv::CV_64FC1); t_currCam_prevCam_ = uvocv::Mat::zeros(3, 1, uvocv::CV_64FC1);
        rvec_ = uvocv::Mat::zeros(3, 1, uvocv::CV_64FC1); t_prevCam_currCam_ = uvocv::Mat::zeros(3, 1, uvocv::CV_64FC1);
    }

    // frames submitted and not collected are collected (their results dropped) before the node's copies of their pixels go
    ~visual_odometry_core() { Published p; while (!fifo_.empty()) { try { spin_collect(p); } catch (...) {} } }
    visual_odometry_core(const visual_odometry_core&) = delete;
    visual_odometry_core& operator=(const visual_odometry_core&) = delete;

    // ---- the subscribers' callbacks (queue size 1: the newest message replaces an unprocessed one) ----
    void mono_imgs_callback(const uvocv::Mat& img, double stamp) { camera_img_ = img; dev_img_ = DeviceImage(); drop_messages(); stamp_ = stamp; first_img_ = true; new_img_available_ = true; }   // VO:67-73
    void range_callback(double range) { range_ = range; }                                                                                               // VO:75-78
    void stereo_imgs_callback(const uvocv::Mat& left, const uvocv::Mat& right, double stamp)                                                            // VO:88-95
    { camera_left_ = left; camera_right_ = right; dev_left_ = dev_right_ = DeviceImage(); drop_messages(); stamp_ = stamp; first_img_ = true; new_img_available_ = true; }
    // The same callbacks for images that are already in the GPU's memory (decode_compressed_image_device, image_codec.h): the fused
    // iterations read them in place; the operator loops take host Mats, so Execution::operators copies them down once, here.
    void mono_imgs_callback(const DeviceImage& img, double stamp)
    {
        if (exec_ == Execution::operators) { mono_imgs_callback(img.download(), stamp); return; }
        dev_img_ = img; camera_img_ = Mat(); drop_messages(); stamp_ = stamp; first_img_ = true; new_img_available_ = true;
    }
    void stereo_imgs_callback(const DeviceImage& left, const DeviceImage& right, double stamp)
    {
        if (exec_ == Execution::operators) { stereo_imgs_callback(left.download(), right.download(), stamp); return; }
        dev_left_ = left; dev_right_ = right; camera_left_ = Mat(); camera_right_ = Mat(); drop_messages(); stamp_ = stamp; first_img_ = true; new_img_available_ = true;
    }
    // The same callbacks for the compressed messages themselves: the fused iterations hand them to the compressed loop entries;
    // Execution::operators decodes them to host Mats, here, as from_ros_to_cv_image does.
    void mono_imgs_callback(const CompressedMessage& msg, double stamp)
    {
        if (exec_ == Execution::operators) { mono_imgs_callback(decode_compressed_image(msg.data.data(), msg.data.size(), msg.format), stamp); return; }
        msg_[0] = msg; msg_[1] = CompressedMessage(); camera_img_ = Mat(); dev_img_ = DeviceImage(); stamp_ = stamp; first_img_ = true; new_img_available_ = true;
    }
    void stereo_imgs_callback(const CompressedMessage& left, const CompressedMessage& right, double stamp)
    {
        if (exec_ == Execution::operators) {
            stereo_imgs_callback(decode_compressed_image(left.data.data(), left.data.size(), left.format), decode_compressed_image(right.data.data(), right.data.size(), right.format), stamp);
            return;
        }
        msg_[0] = left; msg_[1] = right; camera_left_ = Mat(); camera_right_ = Mat(); dev_left_ = dev_right_ = DeviceImage(); stamp_ = stamp; first_img_ = true; new_img_available_ = true;
    }
    // compressed messages that went through decode_compressed_image_device and the frames entry because the compressed entry refused their kind
    int compressed_fallbacks() const { return compressed_fallbacks_; }
    // What a 1-channel frame (Mat or DeviceImage) is: UVO_PIX_BAYER_BGGR8 makes it a BGGR mosaic, demosaiced inside get_image in all
    // three execution modes; under the default, UVO_PIX_BGR8, 1-channel frames are refused as before.  3-channel frames are always BGR8
    // and 4-channel frames BGRA8 (cv_bridge's Mat for an RGBA PNG topic: the first three channels count).  Both cameras of a pair share
    // one layout, and the layout of a topic cannot change while frames are in flight (spin_collect first).
    void set_pixel_format(int fmt)
    {
        if (fmt != UVO_PIX_BGR8 && fmt != UVO_PIX_BAYER_BGGR8) throw Error(UVO_INVALID_ARG, "set_pixel_format: UVO_PIX_BGR8 (colour frames by their channel count) or UVO_PIX_BAYER_BGGR8 (1-channel frames are mosaics)");
        if (!fifo_.empty()) throw Error(UVO_INVALID_ARG, "set_pixel_format: frames are in flight (spin_collect first)");
        pixel_format_ = fmt;
    }
    int pixel_format() const { return pixel_format_; }

    // ---- one iteration of the node's loop (after ros::spinOnce(); loop_rate.sleep()) ----
    Published spin_once()
    {
        if (exec_ == Execution::fused) return fused_iteration();
        return mode_ == "stereo" ? stereo_iteration() : mono_iteration();
    }
    bool initialized() const { return vo_initialized_; }
    Execution execution() const { return exec_; }

    // ---- pipelined replay (Execution::fused only): for recorded sequences, where throughput counts and latency does not ----
    // Up to `depth` frames in flight (1..16, default 2; uvo_stereo_set_depth: the stereo loop is fastest at 6).  Not with frames in flight.
    void set_depth(int depth)
    {
        need_fused("set_depth");
        if (depth < 1 || depth > 16) throw Error(UVO_INVALID_ARG, "set_depth: 1..16");
        if (!fifo_.empty()) throw Error(UVO_INVALID_ARG, "set_depth: frames are in flight (spin_collect first)");
        loop_set_depth(mode_ == "mono" && depth < 2 ? 2 : depth);        // a mono frame is matched against the previous lane's buffers: two lanes at least
        depth_ = depth; depth_set_ = true;
    }
    // Takes the frame the callbacks last delivered and queues its iteration; false when there is none.  The node keeps the frame (a
    // cv::Mat header on the caller's pixels: they must stay unmodified until the frame's spin_collect).
    bool spin_submit()
    {
        need_fused("spin_submit");
        if (!first_img_) return false;
        fused_setup();
        if (!new_img_available_) return false;
        if ((int)fifo_.size() >= depth_) throw Error(UVO_INVALID_ARG, "spin_submit: the pipeline is full (spin_collect first, or set_depth)");
        if (!depth_set_) set_depth(depth_);
        fifo_.push_back(take_frame());
        Frame& f = fifo_.back();
        try {
            if (mode_ == "stereo")
                enter(f, [&] { loop_stereo_submit_compressed(f.msg[0].data.data(), f.msg[0].data.size(), f.msg[1].data.data(), f.msg[1].data.size(), f.msg[0].format, f.msg[1].format); },
                      [&] { stereo_submit_frames(f.p[0], f.p[1], f.w, f.h, f.stride, f.mem); });
            else
                enter(f, [&] { loop_mono_submit_compressed(f.msg[0].data.data(), f.msg[0].data.size(), f.msg[0].format, (double)(float)f.range); },
                      [&] { mono_submit_frames(f.p[0], f.w, f.h, f.stride, f.mem, (double)(float)f.range); });
        } catch (...) { fifo_.pop_back(); throw; }
        f.msg[0] = f.msg[1] = CompressedMessage();                       // the entry consumed the payloads: nothing of them is kept until the collect
        new_img_available_ = false;
        return true;
    }
    // The oldest frame in flight: what spin_once() publishes for it (results come in the order of submission); false when none is.
    bool spin_collect(Published& out)
    {
        if (fifo_.empty()) return false;
        const Frame f = fifo_.front();
        fifo_.pop_front();                                               // the library dequeues the entry whether its collect succeeds or not
        out = fused_collect(f);
        return true;
    }
    int in_flight() const { return (int)fifo_.size(); }

private:
    using Mat = uvocv::Mat;
    std::string mode_;
    Execution exec_ = Execution::operators;
    bool first_img_ = false, new_img_available_ = false, vo_initialized_ = false, cameras_ready_ = false;
    double range_ = 1.0, stamp_ = 0, prev_time_ = 0;
    Mat camera_img_, camera_left_, camera_right_;
    // mono state (VO:196-214)
    Mat camera_matrix_, distortion_, new_camera_matrix_, prev_projection_matrix_;
    Mat R_currCam_prevCam_, t_currCam_prevCam_;
    double SF_ = 1.0;
    std::vector<uvocv::KeyPoint> prev_keypoints_; Mat prev_descriptors_;
    // stereo state (VO:424-470)
    Mat K_left_, K_right_, dist_left_, dist_right_, newK_left_, newK_right_, P_eye_left_, P_right_;
    Mat rvec_, t_prevCam_currCam_;
    std::vector<uvocv::DMatch> results_match_prev_;
    std::vector<uvocv::KeyPoint> prevL_as_, prevR_as_; Mat prevL_desc_as_;

    // fused execution: the frame as the loop entry takes it, and the frames in flight in the order of their submission
    struct Frame {
        Mat host[2]; DeviceImage dev[2];                                 // keep the pixels alive until the collect
        CompressedMessage msg[2];                                        // a compressed frame: the payloads, until its entry has consumed them
        const unsigned char* p[2] = {nullptr, nullptr};
        int w = 0, h = 0, stride = 0, mem = UVO_MEM_HOST;
        int fmt = UVO_PIX_BGR8;                                          // the pixels' layout, from their channel count (layout_of)
        double stamp = 0, range = 0;
    };
    int pixel_format_ = UVO_PIX_BGR8;                                    // set_pixel_format: what a 1-channel frame is
    int ctx_format_ = -1;                                                // the layout the context's cameras were last given (-1: not yet)
    // the layout of a frame with `channels` channels, -1 when the node does not take it
    int layout_of(int channels) const
    { return channels == 3 ? UVO_PIX_BGR8 : channels == 4 ? UVO_PIX_BGRA8 : (channels == 1 && pixel_format_ == UVO_PIX_BAYER_BGGR8) ? UVO_PIX_BAYER_BGGR8 : -1; }
    static int bytes_per_pixel(int fmt) { return fmt == UVO_PIX_BGRA8 ? 4 : fmt == UVO_PIX_BAYER_BGGR8 ? 1 : 3; }
    // the context's cameras read frames in layout fmt from now on (refused by the library while frames are in flight)
    void cameras_read(int fmt)
    {
        if (fmt == ctx_format_) return;
        loop_set_camera_format(0, fmt);
        if (mode_ == "stereo") loop_set_camera_format(1, fmt);
        ctx_format_ = fmt;
    }
    // get_image of the operator loops on whatever layout the node takes
    Mat get_image_any(const Mat& img, const Mat& K, const Mat& dist, const Mat& newK) const
    {
        if (img.type() == uvocv::CV_8UC1 && pixel_format_ == UVO_PIX_BAYER_BGGR8) return get_image_bayer(img, K, dist, newK);
        return get_image(img, K, dist, newK);
    }
    DeviceImage dev_img_, dev_left_, dev_right_;
    CompressedMessage msg_[2];                                           // the compressed message(s) the callbacks last delivered (fused execution)
    int compressed_fallbacks_ = 0;
    void drop_messages() { msg_[0] = msg_[1] = CompressedMessage(); }
    std::deque<Frame> fifo_;
    int depth_ = 2; bool depth_set_ = false;

    static Mat mat33(double a, double b, double c, double d, double e, double f, double g, double h, double i)
    { Mat m(3, 3, uvocv::CV_64FC1); const double v[9] = {a, b, c, d, e, f, g, h, i}; for (int k = 0; k < 9; k++) m.at<double>(k / 3, k % 3) = v[k]; return m; }
    static Mat row4(double a, double b, double c, double d) { Mat m(1, 4, uvocv::CV_64FC1); m.at<double>(0, 0) = a; m.at<double>(0, 1) = b; m.at<double>(0, 2) = c; m.at<double>(0, 3) = d; return m; }
    static std::vector<uvocv::Point2f> points_of(const std::vector<uvocv::KeyPoint>& k) { std::vector<uvocv::Point2f> p; p.reserve(k.size()); for (const auto& q : k) p.push_back(q.pt); return p; }   // KeyPoint::convert

    // ------------------------------------------------------------------ mono_VO (VO:167-398)
    Published mono_iteration()
    {
        Published out;
        if (!first_img_) return out;                                                       // VO:173-177
        if (!cameras_ready_) {                                                             // VO:188-189, 221-225 (once, on the first image)
            distortion_ = row4(k1, k2, p1, p2);
            camera_matrix_ = mat33(fx, 0, ccx, 0, fy, ccy, 0, 0, 1);
            resize_camera_matrix(camera_img_, camera_matrix_, distortion_, new_camera_matrix_);
            prev_projection_matrix_ = compute_projection_matrix(Mat::eye(3, 3, uvocv::CV_64FC1), Mat::zeros(3, 1, uvocv::CV_64FC1), new_camera_matrix_);
            cameras_ready_ = true;
        }
        if (!new_img_available_) return out;
        new_img_available_ = false;
        const double curr_time = stamp_;
        Mat curr_img = get_image_any(camera_img_, camera_matrix_, distortion_, new_camera_matrix_);          // VO:235 / VO:260
        std::vector<uvocv::KeyPoint> curr_keypoints; Mat curr_descriptors;
        detect_features(curr_img, curr_keypoints, curr_descriptors);                      // VO:238 / VO:274
        out.n_kps = (int)curr_keypoints.size();
        auto roll = [&]() { prev_keypoints_ = curr_keypoints; prev_descriptors_ = curr_descriptors.clone(); prev_time_ = curr_time; };
        if (!vo_initialized_) {                                                            // VO:227-245
            roll();
            if ((int)curr_keypoints.size() >= MIN_NUM_FEATURES) vo_initialized_ = true;
            return out;
        }
        const double deltaT = curr_time - prev_time_;
        if ((int)curr_keypoints.size() < MIN_NUM_FEATURES) { roll(); return out; }         // VO:276-284
        std::vector<uvocv::DMatch> matches, inlier_matches;
        std::vector<uvocv::Point2f> prev_conv, curr_conv, prev_inliers, curr_inliers;
        match_features(prev_keypoints_, curr_keypoints, prev_descriptors_, curr_descriptors, matches, prev_conv, curr_conv);       // VO:287
        out.n_matches = (int)matches.size();
        if ((int)matches.size() < MIN_NUM_FEATURES) { roll(); return out; }                // VO:299-307
        use_essential = select_estimation_method(prev_conv, curr_conv);                    // VO:310-317
        bool success = false;
        estimate_relative_pose(prev_conv, curr_conv, new_camera_matrix_, R_currCam_prevCam_, t_currCam_prevCam_, prev_inliers, curr_inliers, inlier_matches, success);   // VO:323
        out.n_inliers = (int)prev_inliers.size();
        bool valid = success;                                                              // VO:335-344
        if (success) {                                                                     // VO:351-376
            Mat points4d, good_idx, good_prev;
            Mat curr_projection = compute_projection_matrix(R_currCam_prevCam_, t_currCam_prevCam_, new_camera_matrix_);
            uvo_hip::triangulatePoints(prev_projection_matrix_, curr_projection, prev_inliers, curr_inliers, points4d);
            extract_3Dpoints(prev_inliers, curr_inliers, Mat::eye(3, 3, uvocv::CV_64FC1), Mat::zeros(3, 1, uvocv::CV_64FC1), R_currCam_prevCam_, t_currCam_prevCam_,
                             new_camera_matrix_, new_camera_matrix_, points4d, good_prev, good_idx);
            out.n_good3d = good_prev.rows;
            if (good_prev.rows < MIN_NUM_3DPOINTS) valid = false;                          // VO:358
            else {
                Mat good_curr = convert_3Dpoints_camera(good_prev, R_currCam_prevCam_, t_currCam_prevCam_);
                if (!good_curr.empty()) SF_ = compute_scale_factor((float)range_, good_curr);      // VO:366-368 (range narrows to float)
                else valid = false;
            }
        }
        // mono_output_computation (VO:126-140): -SF * R^T * t / deltaT, evaluated as OpenCV's gemm does: alpha = (-SF) * (1 / deltaT)
        const double alpha = (-SF_) * (1.0 / deltaT);
        for (int i = 0; i < 3; i++) {
            double acc = 0;
            for (int k = 0; k < 3; k++) acc += R_currCam_prevCam_.at<double>(k, i) * t_currCam_prevCam_.at<double>(k, 0);
            out.v[i] = acc * alpha;
        }
        out.published = true; out.valid = valid; out.stamp = curr_time;
        roll();                                                                            // VO:392-395
        return out;
    }

    // ------------------------------------------------------------------ stereo_VO (VO:406-741)
    Published stereo_iteration()
    {
        Published out;
        if (!first_img_) return out;                                                       // VO:412-416
        const Mat R_eye = Mat::eye(3, 3, uvocv::CV_64FC1), t_zeros = Mat::zeros(3, 1, uvocv::CV_64FC1);
        if (!cameras_ready_) {                                                             // VO:426-463
            K_left_ = mat33(fx_left, 0, ccx_left, 0, fy_left, ccy_left, 0, 0, 1); K_right_ = mat33(fx_right, 0, ccx_right, 0, fy_right, ccy_right, 0, 0, 1);
            dist_left_ = row4(k1_left, k2_left, p1_left, p2_left); dist_right_ = row4(k1_right, k2_right, p1_right, p2_right);
            resize_camera_matrix(camera_left_, K_left_, dist_left_, newK_left_);
            resize_camera_matrix(camera_right_, K_right_, dist_right_, newK_right_);
            P_eye_left_ = compute_projection_matrix(R_eye, t_zeros, newK_left_);           // VO:460
            P_right_ = compute_projection_matrix(R_right, t_right, newK_right_);           // VO:462
            cameras_ready_ = true;
        }
        if (!new_img_available_) return out;
        new_img_available_ = false;
        const double curr_time = stamp_;
        Mat L = get_image_any(camera_left_, K_left_, dist_left_, newK_left_), R = get_image_any(camera_right_, K_right_, dist_right_, newK_right_);     // VO:482-483 / 542-543
        std::vector<uvocv::KeyPoint> kL, kR; Mat dL, dR;
        detect_features(L, kL, dL); detect_features(R, kR, dR);                            // VO:486-487 / 548-549
        out.n_kps = (int)kL.size();
        if (!vo_initialized_) {                                                            // VO:474-520
            prev_time_ = curr_time;
            if ((int)kL.size() >= MIN_NUM_FEATURES && (int)kR.size() >= MIN_NUM_FEATURES) {
                match_features(kL, kR, dL, dR, results_match_prev_);                       // appends (VOU:538)
                if ((int)results_match_prev_.size() > MIN_NUM_FEATURES) vo_initialized_ = true;
            }
            if (vo_initialized_) {
                Mat il, ir;
                for (const auto& m : results_match_prev_) { il.push_back(m.queryIdx); ir.push_back(m.trainIdx); }
                select_desired_descriptors(dL, prevL_desc_as_, il); select_desired_keypoints(kL, prevL_as_, il); select_desired_keypoints(kR, prevR_as_, ir);
            }
            return out;
        }
        const double deltaT = curr_time - prev_time_;
        bool valid = false;
        std::vector<uvocv::DMatch> m_curr, m_pc;
        std::vector<uvocv::KeyPoint> currL_as, currR_as; Mat currL_desc_as, good_pts, good_idx, inliers_idx;
        Mat distCoeffs = Mat::zeros(4, 1, uvocv::CV_64FC1), tvec = Mat::zeros(3, 1, uvocv::CV_64FC1);
        if ((int)kL.size() >= MIN_NUM_FEATURES && (int)kR.size() >= MIN_NUM_FEATURES) {    // VO:556
            match_features(kL, kR, dL, dR, m_curr);                                        // VO:558
            if ((int)m_curr.size() > MIN_NUM_FEATURES) {                                   // VO:567
                Mat il, ir;
                for (const auto& m : m_curr) { il.push_back(m.queryIdx); ir.push_back(m.trainIdx); }
                select_desired_descriptors(dL, currL_desc_as, il); select_desired_keypoints(kL, currL_as, il); select_desired_keypoints(kR, currR_as, ir);
                match_features(prevL_as_, kL, prevL_desc_as_, dL, m_pc);                   // VO:592
                Mat pl_idx, cu_idx;
                for (const auto& m : m_pc) { pl_idx.push_back(m.queryIdx); cu_idx.push_back(m.trainIdx); }
                std::vector<uvocv::KeyPoint> pl, pr, cu;
                select_desired_keypoints(prevL_as_, pl, pl_idx); select_desired_keypoints(prevR_as_, pr, pl_idx); select_desired_keypoints(kL, cu, cu_idx);
                std::vector<uvocv::Point2f> x1 = points_of(pl), x2 = points_of(pr);
                if ((int)m_pc.size() > MIN_NUM_FEATURES) {                                 // VO:626
                    Mat points4D;
                    uvo_hip::triangulatePoints(P_eye_left_, P_right_, x1, x2, points4D);   // VO:631
                    extract_3Dpoints(x1, x2, R_eye, t_zeros, R_right, t_right, newK_left_, newK_right_, points4D, good_pts, good_idx);
                    if (good_pts.rows > MIN_NUM_3DPOINTS) {                                // VO:634
                        std::vector<uvocv::KeyPoint> good_cu;
                        select_desired_keypoints(cu, good_cu, good_idx);
                        std::vector<uvocv::Point2f> ci = points_of(good_cu);
                        uvo_hip::solvePnPRansac(good_pts, ci, newK_left_, distCoeffs, rvec_, tvec, USE_EXTRINSIC_GUESS, ITERATIONS_COUNT,
                                                (float)REPROJECTION_ERROR_THRESHOLD, CONFIDENCE, inliers_idx, PNP_METHOD_FLAG);          // VO:647-648
                        if (inliers_idx.rows >= MIN_NUM_INLIERS) {                         // VO:665
                            Mat Rm;
                            uvo_hip::Rodrigues(rvec_, Rm);                                 // VO:673
                            for (int i = 0; i < 3; i++) {                                  // VO:675: t_prevCam_currCam = -R^T t
                                double acc = 0;
                                for (int k = 0; k < 3; k++) acc += Rm.at<double>(k, i) * tvec.at<double>(k, 0);
                                t_prevCam_currCam_.at<double>(i, 0) = acc * -1.0;
                            }
                            valid = true;
                        }
                    }
                }
            }
        }
        out.n_matches = (int)m_pc.size(); out.n_good3d = good_pts.rows; out.n_inliers = inliers_idx.rows;
        for (int i = 0; i < 3; i++) out.v[i] = t_prevCam_currCam_.at<double>(i, 0) / deltaT;             // stereo_output_computation (VO:148-159)
        out.published = true; out.valid = valid; out.stamp = curr_time;
        prevL_as_ = currL_as; prevR_as_ = currR_as; prevL_desc_as_ = currL_desc_as.clone(); prev_time_ = curr_time;     // VO:723-733
        return out;
    }

    // ------------------------------------------------------------------ Execution::fused
    void need_fused(const char* who) const
    { if (exec_ != Execution::fused) throw Error(UVO_INVALID_ARG, std::string(who) + ": the node was built with Execution::operators (pass Execution::fused)"); }

    // the frame the callbacks last delivered, as the camera-frames entries take it
    Frame take_frame() const
    {
        Frame f;
        const bool stereo = mode_ == "stereo";
        const int ncam = stereo ? 2 : 1;
        f.stamp = stamp_; f.range = range_;
        if (!msg_[0].data.empty()) {
            for (int i = 0; i < ncam; i++) {
                if (msg_[i].data.empty()) throw Error(UVO_INVALID_ARG, "fused iteration: an empty compressed message");
                f.msg[i] = msg_[i];
            }
            return f;
        }
        if (!(stereo ? dev_left_ : dev_img_).empty()) {
            f.dev[0] = stereo ? dev_left_ : dev_img_; if (stereo) f.dev[1] = dev_right_;
            take_device(f, ncam);
            return f;
        }
        f.host[0] = stereo ? camera_left_ : camera_img_; if (stereo) f.host[1] = camera_right_;
        auto channels_of = [](const Mat& m) { return m.type() == uvocv::CV_8UC3 ? 3 : m.type() == uvocv::CV_8UC4 ? 4 : m.type() == uvocv::CV_8UC1 ? 1 : 0; };
        f.fmt = f.host[0].empty() ? -1 : layout_of(channels_of(f.host[0]));
        const int bpp = bytes_per_pixel(f.fmt);
        auto pitch = [bpp](const Mat& m) { return m.rows > 1 ? (int)(m.ptr<unsigned char>(1) - m.ptr<unsigned char>(0)) : m.cols * bpp; };     // rows may be padded in a real cv::Mat
        for (int i = 0; i < ncam; i++)
            if (f.fmt < 0 || f.host[i].empty() || f.host[i].type() != f.host[0].type() || f.host[i].cols != f.host[0].cols || f.host[i].rows != f.host[0].rows)
                throw Error(UVO_INVALID_ARG, "fused iteration: CV_8UC3 or CV_8UC4 images (CV_8UC1 mosaics under set_pixel_format) of one size and type expected");
        if (stereo && pitch(f.host[0]) != pitch(f.host[1])) { f.host[0] = f.host[0].clone(); f.host[1] = f.host[1].clone(); }       // the entry takes one pitch for the pair: clone() packs the rows
        for (int i = 0; i < ncam; i++) f.p[i] = f.host[i].ptr<unsigned char>(0);
        f.w = f.host[0].cols; f.h = f.host[0].rows; f.stride = pitch(f.host[0]); f.mem = UVO_MEM_HOST;
        return f;
    }

    // the frame's device images, as the frames entries take them: one size, one layout
    void take_device(Frame& f, int ncam) const
    {
        f.fmt = f.dev[0].empty() ? -1 : layout_of(f.dev[0].channels);
        for (int i = 0; i < ncam; i++) {
            if (f.fmt < 0 || f.dev[i].empty() || f.dev[i].channels != f.dev[0].channels || f.dev[i].cols != f.dev[0].cols || f.dev[i].rows != f.dev[0].rows)
                throw Error(UVO_INVALID_ARG, "fused iteration: 3- or 4-channel device images (1-channel mosaics under set_pixel_format) of one size and layout expected");
            f.p[i] = f.dev[i].data();
        }
        f.w = f.dev[0].cols; f.h = f.dev[0].rows; f.stride = f.w * bytes_per_pixel(f.fmt); f.mem = UVO_MEM_DEVICE;
    }

    // A frame into its loop entry: `frames` for pixels; for compressed messages `compressed`, and when that entry refuses the payload
    // by kind (its "compressed entry:" refusals: a PNG, a decode that does not give three channels -- made before anything is queued),
    // decode_compressed_image_device followed by `frames`
    template <class Compressed, class Frames>
    void enter(Frame& f, Compressed&& compressed, Frames&& frames)
    {
        if (f.msg[0].data.empty()) { cameras_read(f.fmt); frames(); return; }
        try { compressed(); return; }
        catch (const Error& e) { if (e.status != UVO_INVALID_ARG || std::string(e.what()).find("compressed entry:") == std::string::npos) throw; }
        const int ncam = mode_ == "stereo" ? 2 : 1;
        for (int i = 0; i < ncam; i++) f.dev[i] = decode_compressed_image_device(f.msg[i].data.data(), f.msg[i].data.size(), f.msg[i].format);
        take_device(f, ncam);                                            // an RGBA PNG decodes to four channels: BGRA8
        compressed_fallbacks_++;
        cameras_read(f.fmt);
        frames();
    }
    // the size of a compressed message's picture, from its headers
    static Mat size_of_message(const CompressedMessage& m)
    {
        int w = 0, h = 0, ch = 0;
        uvo_ctx* c = context();
        const uvo_status st = uvo_decode_image(c, m.data.data(), m.data.size(), m.format.c_str(), nullptr, 0, UVO_MEM_HOST, &w, &h, &ch);
        if (st != UVO_OK) throw Error(st, std::string("uvo_decode_image: ") + uvo_last_error(c));
        return Mat(h, w, uvocv::CV_8UC1);
    }

    // once, on the first image (VO:188-189, 221-225 mono; VO:426-463 stereo): the cameras, the rig, the detector and the PnP method
    // (PNP_METHOD_FLAG reaches the context with the other parameter globals, in every shim call) go to the context
    void fused_setup()
    {
        if (cameras_ready_) return;
        const bool stereo = mode_ == "stereo";
        const DeviceImage& d0 = stereo ? dev_left_ : dev_img_;
        // resize_camera_matrix reads the size of the original image only
        const bool compressed = !msg_[0].data.empty();
        auto size_of = [&](int cam, const Mat& m, const DeviceImage& d) { return compressed ? size_of_message(msg_[cam]) : (d.empty() ? m : Mat(d.rows, d.cols, uvocv::CV_8UC1)); };
        if (stereo) {
            K_left_ = mat33(fx_left, 0, ccx_left, 0, fy_left, ccy_left, 0, 0, 1); K_right_ = mat33(fx_right, 0, ccx_right, 0, fy_right, ccy_right, 0, 0, 1);
            dist_left_ = row4(k1_left, k2_left, p1_left, p2_left); dist_right_ = row4(k1_right, k2_right, p1_right, p2_right);
            resize_camera_matrix(size_of(0, camera_left_, d0), K_left_, dist_left_, newK_left_);
            resize_camera_matrix(size_of(1, camera_right_, dev_right_), K_right_, dist_right_, newK_right_);
            loop_set_camera(0, K_left_, dist_left_, newK_left_);
            loop_set_camera(1, K_right_, dist_right_, newK_right_);
            loop_set_rig(newK_left_, newK_right_, R_right, t_right);
        } else {
            distortion_ = row4(k1, k2, p1, p2);
            camera_matrix_ = mat33(fx, 0, ccx, 0, fy, ccy, 0, 0, 1);
            resize_camera_matrix(size_of(0, camera_img_, d0), camera_matrix_, distortion_, new_camera_matrix_);
            loop_set_camera(0, camera_matrix_, distortion_, new_camera_matrix_);
            loop_set_mono_camera(new_camera_matrix_);
        }
        loop_reset(stereo);                                              // the shared context may hold an earlier node's sequence
        ctx_format_ = -1; cameras_read(UVO_PIX_BGR8);                    // ... and its cameras' layout
        loop_set_detector();
        cameras_ready_ = true;
    }

    Published fused_iteration()
    {
        Published out;
        if (!first_img_) return out;                                     // VO:173-177 / VO:412-416
        fused_setup();
        if (!new_img_available_) return out;
        if (!fifo_.empty()) throw Error(UVO_INVALID_ARG, "spin_once: frames submitted with spin_submit are in flight (spin_collect first)");
        new_img_available_ = false;
        Frame f = take_frame();
        const double dt = f.stamp - prev_time_;
        prev_time_ = f.stamp;
        if (mode_ == "stereo") {
            uvo_stereo_result r;
            enter(f, [&] { loop_stereo_step_compressed(f.msg[0].data.data(), f.msg[0].data.size(), f.msg[1].data.data(), f.msg[1].data.size(), f.msg[0].format, f.msg[1].format, dt, r); },
                  [&] { stereo_step_frames(f.p[0], f.p[1], f.w, f.h, f.stride, f.mem, dt, r); });
            return published_of(r, f.stamp);
        }
        uvo_mono_result r;
        enter(f, [&] { loop_mono_step_compressed(f.msg[0].data.data(), f.msg[0].data.size(), f.msg[0].format, (double)(float)f.range, dt, r); },
              [&] { mono_step_frames(f.p[0], f.w, f.h, f.stride, f.mem, (double)(float)f.range, dt, r); });      // VO:366-368 (range narrows to float)
        return published_of(r, f.stamp);
    }
    // the collect of the oldest submitted frame: deltaT is its stamp minus its predecessor's, as in the synchronous loop
    Published fused_collect(const Frame& f)
    {
        const double dt = f.stamp - prev_time_;
        prev_time_ = f.stamp;
        if (mode_ == "stereo") { uvo_stereo_result r; stereo_collect(dt, r); return published_of(r, f.stamp); }
        uvo_mono_result r; mono_collect(dt, r); return published_of(r, f.stamp);
    }

    // what stereo_iteration() reports, from the loop entry's result: nothing is published for a pair the init loop consumed (VO:474-520)
    Published published_of(const uvo_stereo_result& r, double stamp)
    {
        Published out;
        out.n_kps = r.n_left;
        if (!r.initialized) {
            vo_initialized_ = r.n_left >= MIN_NUM_FEATURES && r.n_right >= MIN_NUM_FEATURES && r.n_stereo_matches > MIN_NUM_FEATURES;
            return out;
        }
        vo_initialized_ = true;
        out.n_matches = r.n_tri_matches; out.n_good3d = r.n_good3d; out.n_inliers = r.n_inliers;
        for (int i = 0; i < 3; i++) out.v[i] = r.velocity[i];
        out.published = true; out.valid = r.valid != 0; out.stamp = stamp;
        return out;
    }
    // what mono_iteration() reports: a frame skipped with `continue` (VO:276-307) or consumed by the init loop publishes nothing
    Published published_of(const uvo_mono_result& r, double stamp)
    {
        Published out;
        out.n_kps = r.n_kps; out.n_matches = r.n_matches; out.n_inliers = r.n_inliers; out.n_good3d = r.n_good3d;
        vo_initialized_ = vo_initialized_ || r.initialized || r.n_kps >= MIN_NUM_FEATURES;
        if (!r.published) return out;
        use_essential = r.used_essential != 0;                           // the reference's global: written where the operator loop writes it (VO:310-317, VOU:160-163)
        for (int i = 0; i < 3; i++) out.v[i] = r.velocity[i];
        out.published = true; out.valid = r.valid != 0; out.stamp = stamp;
        return out;
    }
};

}  // namespace uvo_hip
