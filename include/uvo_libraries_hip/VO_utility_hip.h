// VO_utility_hip.h -- the uvo_libraries function surface, served by libuvo_hip.so (MI355X).
//
// Drop-in for the hot-path part of uvo_libraries/include/uvo_libraries/VO_utility.h (functions VOH:96-117, parameter
// globals VOH:25-89): same names, same argument order and meaning, same in/out conventions (outputs that the
// reference fills with push_back are appended to here as well).  The nodes (uvo/include/visual_odometry.h) include
// this header instead and link libuvo_libraries_hip.so; INTEGRATION.md lists the three lines that change.
//
// Differences a maintainer should know about:
//   * the parameter globals are DECLARED here and DEFINED once in the library (the reference defines them in its
//     header); get_VO_parameters() keeps assigning to them as before, every call below reads their current value;
//   * detect_features serves all four names of FEATURE_DETECTOR; "ORB" needs OpenCV's learned sampling table bit_pattern_31_
//     (features2d/src/orb.cpp), which this library cannot restate: uvo_hip::set_orb_pattern(table), or the environment variable
//     UVO_ORB_PATTERN_FILE naming a text file of its 1024 integers -- without it the ORB branch throws and says so;
//   * OpenCV errors become uvo_hip::Error (a std::runtime_error) carrying the library's message;
//   * the cv:: calls the stereo/mono loops make directly (triangulatePoints, solvePnPRansac, Rodrigues) have
//     same-signature replacements in namespace uvo_hip.
#pragma once
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "uvo_libraries_hip/cv_compat.h"
#include "uvo_hip.h"

// ---- parameter globals (VOH:25-89), defined in VO_utility_hip.cpp ---------------------------------------------
extern std::string FEATURE_DETECTOR;
extern int    DESIRED_WIDTH;              extern bool CLAHE_CORRECTION;   extern int CLIP_LIMIT;      // VOH:41-44
extern int    DISTANCE;
extern int    ESSENTIAL_OUTLIER_METHOD;   extern double ESSENTIAL_MAX_ITERS, ESSENTIAL_CONFIDENCE, ESSENTIAL_THRESHOLD;
extern int    HOMOGRAPHY_OUTLIER_METHOD;  extern double HOMOGRAPHY_MAX_ITERS, HOMOGRAPHY_CONFIDENCE, HOMOGRAPHY_THRESHOLD, HOMOGRAPHY_DISTANCE;
extern double VPF_THRESHOLD, REPROJECTION_TOLERANCE, LOWE_RATIO_THRESHOLD;
extern int    MIN_NUM_FEATURES, MIN_NUM_3DPOINTS, MIN_NUM_INLIERS;
extern int    ITERATIONS_COUNT;           extern double REPROJECTION_ERROR_THRESHOLD, CONFIDENCE;
extern bool   USE_EXTRINSIC_GUESS;        extern int PNP_METHOD_FLAG;
extern int    SURF_MIN_HESSIAN, SURF_OCTAVES_NUMBER, SURF_OCTAVES_LAYERS;
extern bool   SURF_EXTENDED, SURF_UPRIGHT;
extern bool   use_essential;

// ---- functions (VOH:96-117; implementation lines cite uvo_libraries/src/VO_utility.cpp = VOU) ------------------
uvocv::Mat compute_projection_matrix(const uvocv::Mat& R, const uvocv::Mat& t, const uvocv::Mat& cameraIntrinsic);      // VOU:9-15
double     compute_scale_factor(float distance, const uvocv::Mat& world_points);                                        // VOU:23-38
uvocv::Mat convert_3Dpoints_camera(const uvocv::Mat& points_to_convert, const uvocv::Mat& R_to_from, const uvocv::Mat& t_to_from); // VOU:46-63
uvocv::Mat convert_from_homogeneous_coords(const uvocv::Mat& points4d);                                                 // VOU:71-83
// VO_utility.h:112: scales cameraMatrix in place by original width / DESIRED_WIDTH, newCamMatrix = getOptimalNewCameraMatrix(alpha = 0)
void resize_camera_matrix(uvocv::Mat original_image, uvocv::Mat& cameraMatrix, uvocv::Mat distortionCoeff, uvocv::Mat& newCamMatrix);
uvocv::Mat get_image(const uvocv::Mat& current_img, const uvocv::Mat& cameraMatrix, const uvocv::Mat& distortionCoeff,
                     const uvocv::Mat& newCamMatrix);                                                                  // VOU:337-379: CV_8UC3, or CV_8UC4 by its first three channels
void detect_features(uvocv::Mat img, std::vector<uvocv::KeyPoint>& keypoints, uvocv::Mat& descriptors);                 // VOU:91-126
void estimate_relative_pose(std::vector<uvocv::Point2f> keypoints1_conv, std::vector<uvocv::Point2f> keypoints2_conv,
                            uvocv::Mat cameraMatrix, uvocv::Mat& R_currCam_prevCam, uvocv::Mat& t_currCam_prevCam,
                            std::vector<uvocv::Point2f>& inliers1, std::vector<uvocv::Point2f>& inliers2,
                            std::vector<uvocv::DMatch>& inlier_matches, bool& success);                                 // VOU:134-180
void extract_3Dpoints(std::vector<uvocv::Point2f> keypoints1_conv, std::vector<uvocv::Point2f> keypoints2_conv,
                      uvocv::Mat R1, uvocv::Mat t1, uvocv::Mat R2, uvocv::Mat t2, uvocv::Mat cameraMatrix1,
                      uvocv::Mat cameraMatrix2, uvocv::Mat points4D, uvocv::Mat& very_good_cam1_points,
                      uvocv::Mat& very_good_indexes);                                                                   // VOU:188-237
void extract_3Dpoints_and_reprojection(std::vector<uvocv::Point2f> keypoints1_conv, std::vector<uvocv::Point2f> keypoints2_conv,
                      uvocv::Mat R1, uvocv::Mat t1, uvocv::Mat R2, uvocv::Mat t2, uvocv::Mat cameraMatrix1,
                      uvocv::Mat cameraMatrix2, uvocv::Mat points4D, uvocv::Mat& very_good_cam1_points,
                      uvocv::Mat& very_good_indexes, std::vector<double>& reprojection_errors_vector);                  // VOU:245-298
void extract_inliers(const std::vector<uvocv::Point2f>& keypoints1_conv, const std::vector<uvocv::Point2f>& keypoints2_conv,
                     const uvocv::Mat& mask, std::vector<uvocv::Point2f>& inliers1, std::vector<uvocv::Point2f>& inliers2,
                     std::vector<uvocv::DMatch>& inlier_matches);                                                       // VOU:306-329
void match_features(std::vector<uvocv::KeyPoint> keypoints1, std::vector<uvocv::KeyPoint> keypoints2, uvocv::Mat descriptors1,
                    uvocv::Mat descriptors2, std::vector<uvocv::DMatch>& matches);                                      // VOU:515-543
void match_features(std::vector<uvocv::KeyPoint> keypoints1, std::vector<uvocv::KeyPoint> keypoints2, uvocv::Mat descriptors1,
                    uvocv::Mat descriptors2, std::vector<uvocv::DMatch>& matches,
                    std::vector<uvocv::Point2f>& keypoints1_conv, std::vector<uvocv::Point2f>& keypoints2_conv);        // VOU:551-573
int  recover_pose_homography(uvocv::Mat H, std::vector<uvocv::Point2f> inliers1, std::vector<uvocv::Point2f> inliers2,
                             uvocv::Mat cameraMatrix, uvocv::Mat& R, uvocv::Mat& t);                                    // VOU:581-624
std::vector<double> reproject_errors(const uvocv::Mat& world_points, const uvocv::Mat& R, const uvocv::Mat& t,
                                     const uvocv::Mat& cameraMatrix, const std::vector<uvocv::Point2f>& img_points);    // VOU:632-651
void select_desired_descriptors(const uvocv::Mat& descriptors, uvocv::Mat& descriptors_desired, const uvocv::Mat& indexes);   // VOU:683-697
void select_desired_keypoints(const std::vector<uvocv::KeyPoint>& keypoints, std::vector<uvocv::KeyPoint>& keypoints_desired,
                              const uvocv::Mat& indexes);                                                               // VOU:704-717
bool select_estimation_method(const std::vector<uvocv::Point2f>& keypoints1_conv,
                              const std::vector<uvocv::Point2f>& keypoints2_conv);                                      // VOU:725-748

namespace uvo_hip {

struct Error : std::runtime_error { uvo_status status; Error(uvo_status s, const std::string& m) : std::runtime_error(m), status(s) {} };

// The library keeps one process-wide device context, created on first use for images up to max_w x max_h and
// max_kpts keypoints per image.  Call configure() before the first function to choose other limits or another GPU.
void     configure(int device, int max_w, int max_h, int max_kpts);
uvo_ctx* context();
void     shutdown();
// OpenCV's bit_pattern_31_ for the "ORB" branch of detect_features: 1024 ints, x0, y0, x1, y1 per descriptor bit (nullptr forgets it)
void     set_orb_pattern(const int* pattern1024);
// where the "ORB" branch's retainBest rankings run: 1 the device, 0 the host replay (uvo_orb_set_ranking); results do not depend on it.
// Kept across a rebuilt context, as the table is.
void     set_orb_ranking(int where);
// where the "ORB" branch's counts are read while its rankings run on the device: 1 they stay on the device (no host wait in a detection),
// 0 the host reads them back between launches (uvo_orb_set_counts); results do not depend on it.  Kept across a rebuilt context.
void     set_orb_counts(int where);
// where the "AKAZE" branch's contrast factor, duplicate suppression and refinement run: 1 the device, 0 the host scans
// (uvo_akaze_set_suppression); results do not depend on it.  Kept across a rebuilt context.
void     set_akaze_suppression(int where);
// AKAZE::create's arguments, in its order (uvo_akaze_configure), for the "AKAZE" branch of detect_features, loop_set_detector and the node
// classes: descriptor_type 5 (DESCRIPTOR_MLDB), descriptor_size 0 and descriptor_channels 3 only; threshold finite and > 0; nOctaves 1..4;
// nOctaveLayers 1..4; diffusivity 0 (DIFF_PM_G1), 1 (DIFF_PM_G2), 2 (DIFF_WEICKERT), 3 (DIFF_CHARBONNIER).  Anything else throws uvo_hip::Error
// with the library's message -- from this call when a context lives, else from the first call that makes one and takes the AKAZE branch.
// Kept across a rebuilt context and sent before the first detection.  Not called: AKAZE::create()'s defaults.
void     configure_akaze(int descriptor_type = 5, int descriptor_size = 0, int descriptor_channels = 3, float threshold = 0.001f,
                         int nOctaves = 4, int nOctaveLayers = 4, int diffusivity = 1);
// where estimate_relative_pose's attempts run (uvo_mono_set_pose_stage): 1 every attempt a device-resident chain,
// 0 only a first attempt with the essential matrix, the rest through the host-pointer operators (the definition, the library's default); results do not depend
// on it.  Sent to the context at its next use (refused there while frames are in flight).  Kept across a rebuilt context.
void     set_mono_pose_stage(int where);
// ESSENTIAL_OUTLIER_METHOD / HOMOGRAPHY_OUTLIER_METHOD as the globals hold them: throws Error naming the parameter when the library would refuse
// one at the first estimate (uvo_mono_method_refusal); the mono node class asks once, at start-up
void     check_outlier_methods();

// Replacements for the cv:: functions the node loops call directly (visual_odometry.h:355, 631, 647-648, 673).
void triangulatePoints(const uvocv::Mat& projMatr1, const uvocv::Mat& projMatr2, const std::vector<uvocv::Point2f>& projPoints1,
                       const std::vector<uvocv::Point2f>& projPoints2, uvocv::Mat& points4D);
bool solvePnPRansac(const uvocv::Mat& objectPoints /* N x 3 CV_64F */, const std::vector<uvocv::Point2f>& imagePoints,
                    const uvocv::Mat& cameraMatrix, const uvocv::Mat& distCoeffs /* empty or zeros: images are undistorted upstream */,
                    uvocv::Mat& rvec, uvocv::Mat& tvec, bool useExtrinsicGuess, int iterationsCount, float reprojectionError,
                    double confidence, uvocv::Mat& inliers, int flags);
void Rodrigues(const uvocv::Mat& src, uvocv::Mat& dst);

// ---- the fused loops (uvo_stereo_step / uvo_mono_step and their camera-frames entries, include/uvo_hip.h) for the node class
// (visual_odometry_hip.h, Execution::fused).  They run on the same shared context as the functions above, with the current value
// of the parameter globals applied first, so a global changed between two iterations reaches the loop as it reaches the operators;
// with frames in flight such a change is the library's error ("... cannot change while pairs are in flight").  Every refusal of
// the library becomes an Error carrying its message.
//
// An image in the memory of the context's GPU: what decode_compressed_image_device (image_codec.h) returns and the frames entries
// read in place.  Copies share the block; it is freed when the last copy goes (or left to the process's end when the context went
// first).  rows x cols x channels interleaved bytes, tight pitch.
class DeviceImage {
public:
    int rows = 0, cols = 0, channels = 0;
    DeviceImage() = default;
    DeviceImage(int rows_, int cols_, int channels_);
    bool empty() const { return !mem_ || rows == 0 || cols == 0; }
    unsigned char* data() const { return static_cast<unsigned char*>(mem_.get()); }
    size_t bytes() const { return (size_t)rows * cols * channels; }
    uvocv::Mat download() const;                 // a host copy (CV_8UC1 / CV_8UC3 / CV_8UC4)
private:
    std::shared_ptr<void> mem_;
};

// get_image on a CV_8UC1 BGGR mosaic: what cvtColor(COLOR_BayerBGGR2BGR) (math_utility.cpp:154-173, the "bayer" step) and get_image give
uvocv::Mat get_image_bayer(const uvocv::Mat& mosaic, const uvocv::Mat& cameraMatrix, const uvocv::Mat& distortionCoeff,
                           const uvocv::Mat& newCamMatrix);
void loop_set_camera_format(int cam, int pixel_format);        // UVO_PIX_*: the layout the frames entries read camera `cam`'s frames in (uvo_ctx_set_camera_format)
void loop_set_camera(int cam, const uvocv::Mat& cameraMatrix, const uvocv::Mat& distortionCoeff, const uvocv::Mat& newCamMatrix);   // + DESIRED_WIDTH, CLAHE_CORRECTION, CLIP_LIMIT
void loop_set_rig(const uvocv::Mat& newK_left, const uvocv::Mat& newK_right, const uvocv::Mat& R_right, const uvocv::Mat& t_right);
void loop_set_mono_camera(const uvocv::Mat& newCamMatrix);
void loop_set_detector();                        // FEATURE_DETECTOR; "ORB": the sampling table (set_orb_pattern / UVO_ORB_PATTERN_FILE) goes first
void loop_set_depth(int depth);                  // uvo_stereo_set_depth
void loop_reset(bool stereo);                    // uvo_stereo_reset / uvo_mono_reset: the shared context may have run a sequence for an earlier node
int  loop_pending();                             // uvo_ctx_pending
// frames: h x w x 3 interleaved bytes, `stride` bytes per row, mem = UVO_MEM_HOST or UVO_MEM_DEVICE; a submitted frame stays valid and
// unmodified until its collect
void stereo_step_frames(const unsigned char* left, const unsigned char* right, int w, int h, int stride, int mem, double dt, uvo_stereo_result& out);
void stereo_submit_frames(const unsigned char* left, const unsigned char* right, int w, int h, int stride, int mem);
void stereo_collect(double dt, uvo_stereo_result& out);
void mono_step_frames(const unsigned char* img, int w, int h, int stride, int mem, double range, double dt, uvo_mono_result& out);
void mono_submit_frames(const unsigned char* img, int w, int h, int stride, int mem, double range);
void mono_collect(double dt, uvo_mono_result& out);
// compressed frames (uvo_*_compressed): the payload of a sensor_msgs/CompressedImage and its format string, JPEG decoded on the device
// on the entry's lane.  The payload is consumed before the call returns.  A payload the entries refuse by kind (PNG, grey without a
// bayer format, progressive JPEG) throws Error(UVO_INVALID_ARG): decode_compressed_image_device + the frames entry serve those.
void loop_stereo_step_compressed(const unsigned char* left, size_t n_left, const unsigned char* right, size_t n_right, const std::string& format_left, const std::string& format_right, double dt, uvo_stereo_result& out);
void loop_stereo_submit_compressed(const unsigned char* left, size_t n_left, const unsigned char* right, size_t n_right, const std::string& format_left, const std::string& format_right);
void loop_mono_step_compressed(const unsigned char* img, size_t n, const std::string& format, double range, double dt, uvo_mono_result& out);
void loop_mono_submit_compressed(const unsigned char* img, size_t n, const std::string& format, double range);
// uvo_stereo_get / uvo_mono_get of the last collected entry: the element count, or -(count) when cap_bytes is too small
int  stereo_get(const char* what, void* out, int cap_bytes);
int  mono_get(const char* what, void* out, int cap_bytes);

}  // namespace uvo_hip
