// shim_vo_node_exec.cpp -- test driver: shim_vo_node with the node class's execution mode as one more leading argument.
//
//   usage: shim_vo_node_exec <exec> <mono|stereo> <camera_name> <frames.bin> <out.bin> <params.yaml> <intrinsics.yaml> [options]
//   exec      : operators | fused | pipelined:<depth>   (pipelined = Execution::fused through spin_submit / spin_collect)
//   frames.bin, out.bin: as shim_vo_node (one record per frame, in the order of the frames)
//   options   : --dump-image <file>   fused / pipelined: also write uvo_stereo_get("img_left") / uvo_mono_get("img") of the last collected
//                                     frame -- the detector's image, which only a camera-frames entry leaves behind
//               --jpeg host|device    frames.bin holds compressed images instead of pixels: per image int32 nbytes + the payload of a
//                                     sensor_msgs/CompressedImage ("bgr8; jpeg compressed bgr8"), decoded into a host Mat
//                                     (decode_compressed_image) or left in the GPU's memory (decode_compressed_image_device)
//               --time <blocks>       measurement (tools/prof_node.py): <exec> is a comma-separated list; per block and mode a new node runs the
//                                     sequence once untimed (it initialises there) and eight times timed; out.bin becomes a text file of
//                                     "<exec> <ms per iteration>" lines, one per block and mode, after one whole untimed round
//   --config-only as first argument: exactly shim_vo_node's.
#include <chrono>
#include <memory>
#include <string>

#define main shim_vo_node_main             // the existing driver's dump_config() and read_rgb(), not its main()
#include "shim_vo_node.cpp"
#undef main
#include "uvo_libraries_hip/image_codec.h"

namespace {

struct Exec { uvo_hip::Execution exec = uvo_hip::Execution::operators; int depth = 0; std::string name; };     // depth > 0: pipelined

bool parse_exec(const std::string& s, Exec& e)
{
    e = Exec(); e.name = s;
    if (s == "operators") return true;
    e.exec = uvo_hip::Execution::fused;
    if (s == "fused") return true;
    if (s.rfind("pipelined:", 0) != 0) return false;
    e.depth = atoi(s.c_str() + 10);
    return e.depth >= 1 && e.depth <= 16;
}

const int kTimedPasses = 8;                 // --time: passes over the sequence per timed block (a pipeline's fill and drain are in it once)

struct Input { double stamp = 0, range = 0; Mat img[2]; uvo_hip::DeviceImage dev[2]; };

bool read_payload(FILE* f, std::vector<unsigned char>& buf)
{
    int nb = 0;
    if (fread(&nb, sizeof(int), 1, f) != 1 || nb <= 0 || nb > (64 << 20)) return false;
    buf.resize((size_t)nb);
    return fread(buf.data(), 1, buf.size(), f) == buf.size();
}

// jpeg: 0 pixels, 1 decode to a host Mat, 2 decode to device memory
bool read_input(FILE* f, int W, int H, bool stereo, int jpeg, Input& in)
{
    double meta[2];
    if (fread(meta, sizeof(double), 2, f) != 2) return false;
    in.stamp = meta[0]; in.range = meta[1];
    std::vector<unsigned char> buf;
    for (int i = 0; i < (stereo ? 2 : 1); i++) {
        if (jpeg == 0) { if (!read_rgb(f, W, H, in.img[i])) return false; continue; }
        if (!read_payload(f, buf)) return false;
        const std::string fmt = "bgr8; jpeg compressed bgr8";
        if (jpeg == 1) in.img[i] = uvo_hip::decode_compressed_image(buf.data(), buf.size(), fmt);
        else in.dev[i] = uvo_hip::decode_compressed_image_device(buf.data(), buf.size(), fmt);
    }
    return true;
}

void deliver(uvo_hip::visual_odometry_core& node, bool stereo, const Input& in, double stamp)
{
    if (stereo) { if (!in.dev[0].empty()) node.stereo_imgs_callback(in.dev[0], in.dev[1], stamp); else node.stereo_imgs_callback(in.img[0], in.img[1], stamp); }
    else { node.range_callback(in.range); if (!in.dev[0].empty()) node.mono_imgs_callback(in.dev[0], stamp); else node.mono_imgs_callback(in.img[0], stamp); }
}

void write_record(FILE* out, const uvo_hip::Published& p)
{
    const int rec[6] = { p.published, p.valid, p.n_kps, p.n_matches, p.n_inliers, p.n_good3d };
    const double vals[4] = { p.v[0], p.v[1], p.v[2], p.stamp };
    fwrite(rec, sizeof(int), 6, out); fwrite(vals, sizeof(double), 4, out);
}

// one frame through the node in its mode; `sink` receives every record that becomes available (pipelined: of an earlier frame)
template <class Sink>
void feed(uvo_hip::visual_odometry_core& node, const Exec& e, bool stereo, const Input& in, double stamp, Sink&& sink)
{
    deliver(node, stereo, in, stamp);
    if (e.depth == 0) { sink(node.spin_once()); return; }
    uvo_hip::Published p;
    if (node.in_flight() >= e.depth && node.spin_collect(p)) sink(p);
    if (!node.spin_submit()) throw uvo_hip::Error(UVO_INVALID_ARG, "spin_submit took no frame");
}
template <class Sink>
void drain(uvo_hip::visual_odometry_core& node, Sink&& sink) { uvo_hip::Published p; while (node.spin_collect(p)) sink(p); }

}  // namespace

int main(int argc, char** argv)
{
    try {
        if (argc >= 5 && strcmp(argv[1], "--config-only") == 0) return dump_config(argc, argv);
        if (argc < 8) {
            fprintf(stderr, "usage: %s operators|fused|pipelined:<depth> mono|stereo camera frames.bin out.bin params.yaml intrinsics.yaml "
                            "[--dump-image file] [--jpeg host|device] [--time blocks]\n", argv[0]);
            return 2;
        }
        const char* dump_path = nullptr; int jpeg = 0, blocks = 0;
        for (int i = 8; i < argc; i++) {
            if (strcmp(argv[i], "--dump-image") == 0 && i + 1 < argc) dump_path = argv[++i];
            else if (strcmp(argv[i], "--jpeg") == 0 && i + 1 < argc) { const std::string v = argv[++i]; jpeg = v == "device" ? 2 : (v == "host" ? 1 : -1); }
            else if (strcmp(argv[i], "--time") == 0 && i + 1 < argc) blocks = atoi(argv[++i]);
            else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
        }
        if (jpeg < 0) { fprintf(stderr, "--jpeg host|device\n"); return 2; }
        std::vector<Exec> modes;
        for (std::string list = argv[1]; !list.empty();) {
            const size_t comma = list.find(',');
            Exec e;
            if (!parse_exec(list.substr(0, comma), e)) { fprintf(stderr, "exec: operators, fused or pipelined:<1..16>, not '%s'\n", list.substr(0, comma).c_str()); return 2; }
            modes.push_back(e);
            list = comma == std::string::npos ? "" : list.substr(comma + 1);
        }
        if (modes.empty() || (modes.size() > 1 && blocks <= 0)) { fprintf(stderr, "one exec mode (a list only with --time)\n"); return 2; }
        const std::string mode = argv[2];
        const bool stereo = mode == "stereo";
        uvo_hip::ParamTree tree;
        tree.load_yaml_file(argv[6]); tree.load_yaml_file(argv[7]);
        FILE* f = fopen(argv[4], "rb");
        if (!f) { perror("frames"); return 2; }
        int hdr[3];
        if (fread(hdr, sizeof(int), 3, f) != 3) { fprintf(stderr, "short header\n"); return 2; }
        const int W = hdr[0], H = hdr[1], n = hdr[2];
        const int max_kpts = getenv("UVO_TEST_MAX_KPTS") ? atoi(getenv("UVO_TEST_MAX_KPTS")) : 8192;
        uvo_hip::configure(0, W > 640 ? W : 640, H > 480 ? H : 480, max_kpts);
        FILE* out = fopen(argv[5], "wb");
        if (!out) { perror("out"); return 2; }

        if (blocks > 0) {                                                   // ---- measurement
            std::vector<Input> seq((size_t)n);
            for (int k = 0; k < n; k++) if (!read_input(f, W, H, stereo, jpeg, seq[(size_t)k])) { fprintf(stderr, "short frame\n"); return 2; }
            auto nothing = [](const uvo_hip::Published&) {};
            for (int b = -1; b < blocks; b++)                               // block -1: one whole round untimed
                for (const Exec& e : modes) {
                    uvo_hip::visual_odometry_core node(mode, tree, argv[3], e.exec);
                    if (e.depth) node.set_depth(e.depth);
                    double stamp = 1.0;
                    for (int k = 0; k < n; k++) feed(node, e, stereo, seq[(size_t)k], stamp += 0.05, nothing);
                    drain(node, nothing);
                    const auto t0 = std::chrono::steady_clock::now();
                    for (int pass = 0; pass < kTimedPasses; pass++)
                        for (int k = 0; k < n; k++) feed(node, e, stereo, seq[(size_t)k], stamp += 0.05, nothing);
                    drain(node, nothing);
                    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                    if (b >= 0) fprintf(out, "%s %.6f\n", e.name.c_str(), ms / (kTimedPasses * n));
                }
            fclose(out); fclose(f);
            uvo_hip::shutdown();
            return 0;
        }

        const Exec e = modes[0];
        {
            uvo_hip::visual_odometry_core node(mode, tree, argv[3], e.exec);
            if (e.depth) node.set_depth(e.depth);
            auto record = [&](const uvo_hip::Published& p) { write_record(out, p); };
            for (int k = 0; k < n; k++) {
                Input in;                                                   // a new Mat per frame: the node holds a submitted frame's until its collect
                if (!read_input(f, W, H, stereo, jpeg, in)) { fprintf(stderr, "short frame\n"); return 2; }
                feed(node, e, stereo, in, in.stamp, record);
            }
            drain(node, record);
            if (dump_path) {
                const char* key = stereo ? "img_left" : "img";
                unsigned char probe = 0;
                const int count = stereo ? uvo_hip::stereo_get(key, &probe, 0) : uvo_hip::mono_get(key, &probe, 0);       // -(bytes) with no room
                std::vector<unsigned char> img((size_t)(count < 0 ? -count : 0));
                if (!img.empty()) { if (stereo) uvo_hip::stereo_get(key, img.data(), (int)img.size()); else uvo_hip::mono_get(key, img.data(), (int)img.size()); }
                FILE* d = fopen(dump_path, "wb");
                if (!d) { perror("dump"); return 2; }
                fwrite(img.data(), 1, img.size(), d); fclose(d);
            }
        }
        fclose(out); fclose(f);
        uvo_hip::shutdown();
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
