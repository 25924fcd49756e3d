// shim_vo_node_pixfmt.cpp -- test driver: the node class fed with raw frames of one, three or four channels per pixel, one record per
// frame as shim_vo_node_exec writes them.
//
//   usage: shim_vo_node_pixfmt <exec> <mono|stereo> <camera_name> <frames.bin> <out.bin> <params.yaml> <intrinsics.yaml> <channels> [options]
//   exec      : operators | fused | pipelined:<depth>   (pipelined = Execution::fused through spin_submit / spin_collect)
//   frames.bin: int32 W, H, n; per frame double stamp, range, then per image W * H * channels bytes
//   channels  : 1 (a BGGR mosaic: the node is told set_pixel_format(UVO_PIX_BAYER_BGGR8)), 3 (BGR) or 4 (BGRA)
//   options   : --dump-image <file>   fused / pipelined: write uvo_stereo_get("img_left") / uvo_mono_get("img") of the last collected frame
//   --config-only as first argument: exactly shim_vo_node's.
#include <memory>
#include <string>

#define main shim_vo_node_main             // the existing driver's dump_config(), not its main()
#include "shim_vo_node.cpp"
#undef main

namespace {

struct Exec { uvo_hip::Execution exec = uvo_hip::Execution::operators; int depth = 0; };     // depth > 0: pipelined

bool parse_exec(const std::string& s, Exec& e)
{
    e = Exec();
    if (s == "operators") return true;
    e.exec = uvo_hip::Execution::fused;
    if (s == "fused") return true;
    if (s.rfind("pipelined:", 0) != 0) return false;
    e.depth = atoi(s.c_str() + 10);
    return e.depth >= 1 && e.depth <= 16;
}

bool read_frame(FILE* f, int W, int H, int channels, Mat& m)
{
    m = Mat(H, W, channels == 1 ? CV_8UC1 : (channels == 4 ? CV_8UC4 : CV_8UC3));
    const size_t n = (size_t)W * H * channels;
    return fread(m.ptr<uint8_t>(0), 1, n, f) == n;
}

void write_record(FILE* out, const uvo_hip::Published& p)
{
    const int rec[6] = { p.published, p.valid, p.n_kps, p.n_matches, p.n_inliers, p.n_good3d };
    const double vals[4] = { p.v[0], p.v[1], p.v[2], p.stamp };
    fwrite(rec, sizeof(int), 6, out); fwrite(vals, sizeof(double), 4, out);
}

}  // namespace

int main(int argc, char** argv)
{
    try {
        if (argc >= 5 && strcmp(argv[1], "--config-only") == 0) return dump_config(argc, argv);
        if (argc < 9) {
            fprintf(stderr, "usage: %s operators|fused|pipelined:<depth> mono|stereo camera frames.bin out.bin params.yaml intrinsics.yaml 1|3|4 [--dump-image file]\n", argv[0]);
            return 2;
        }
        const char* dump_path = nullptr;
        for (int i = 9; i < argc; i++) {
            if (strcmp(argv[i], "--dump-image") == 0 && i + 1 < argc) dump_path = argv[++i];
            else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
        }
        Exec e;
        if (!parse_exec(argv[1], e)) { fprintf(stderr, "exec: operators, fused or pipelined:<1..16>, not '%s'\n", argv[1]); return 2; }
        const int channels = atoi(argv[8]);
        if (channels != 1 && channels != 3 && channels != 4) { fprintf(stderr, "channels: 1, 3 or 4\n"); return 2; }
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
        {
            uvo_hip::visual_odometry_core node(mode, tree, argv[3], e.exec);
            if (channels == 1) node.set_pixel_format(UVO_PIX_BAYER_BGGR8);
            if (e.depth) node.set_depth(e.depth);
            uvo_hip::Published p;
            for (int k = 0; k < n; k++) {
                double meta[2];
                Mat m[2];                                                   // a new Mat per frame: the node holds a submitted frame's until its collect
                if (fread(meta, sizeof(double), 2, f) != 2) { fprintf(stderr, "short frame\n"); return 2; }
                for (int i = 0; i < (stereo ? 2 : 1); i++) if (!read_frame(f, W, H, channels, m[i])) { fprintf(stderr, "short frame\n"); return 2; }
                if (stereo) node.stereo_imgs_callback(m[0], m[1], meta[0]);
                else { node.range_callback(meta[1]); node.mono_imgs_callback(m[0], meta[0]); }
                if (e.depth == 0) { write_record(out, node.spin_once()); continue; }
                if (node.in_flight() >= e.depth && node.spin_collect(p)) write_record(out, p);
                if (!node.spin_submit()) throw uvo_hip::Error(UVO_INVALID_ARG, "spin_submit took no frame");
            }
            while (node.spin_collect(p)) write_record(out, p);
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
