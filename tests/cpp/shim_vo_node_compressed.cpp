// shim_vo_node_compressed.cpp -- test driver: the node class fed with compressed messages (visual_odometry_core's CompressedMessage
// callbacks), one record per frame as shim_vo_node_exec writes them.
//
//   usage: shim_vo_node_compressed <exec> <mono|stereo> <camera_name> <frames.bin> <out.bin> <params.yaml> <intrinsics.yaml> [options]
//   exec      : operators | fused | pipelined:<depth>   (pipelined = Execution::fused through spin_submit / spin_collect)
//   frames.bin: int32 W, H, n; per frame double stamp, range, then per image int32 nbytes + the payload of a sensor_msgs/CompressedImage
//               (JPEG or PNG; the format string is "bgr8; jpeg compressed bgr8" or "bgr8; png compressed bgr8" by the payload's signature)
//   options   : --dump-image <file>   write uvo_stereo_get("img_left") / uvo_mono_get("img") of the last collected frame
//               --fallbacks <file>    write the node's compressed_fallbacks() as text: messages that took decode + frames entry
//   Every payload buffer is overwritten with 0xFF as soon as the callback has returned: the node keeps its own copy.
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

bool read_message(FILE* f, uvo_hip::CompressedMessage& m)
{
    int nb = 0;
    if (fread(&nb, sizeof(int), 1, f) != 1 || nb <= 0 || nb > (64 << 20)) return false;
    m.data.resize((size_t)nb);
    if (fread(m.data.data(), 1, m.data.size(), f) != m.data.size()) return false;
    const bool png = nb > 4 && m.data[0] == 0x89 && m.data[1] == 'P' && m.data[2] == 'N' && m.data[3] == 'G';
    m.format = png ? "bgr8; png compressed bgr8" : "bgr8; jpeg compressed bgr8";
    return true;
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
        if (argc < 8) {
            fprintf(stderr, "usage: %s operators|fused|pipelined:<depth> mono|stereo camera frames.bin out.bin params.yaml intrinsics.yaml [--dump-image file] [--fallbacks file]\n", argv[0]);
            return 2;
        }
        const char* dump_path = nullptr; const char* fallbacks_path = nullptr;
        for (int i = 8; i < argc; i++) {
            if (strcmp(argv[i], "--dump-image") == 0 && i + 1 < argc) dump_path = argv[++i];
            else if (strcmp(argv[i], "--fallbacks") == 0 && i + 1 < argc) fallbacks_path = argv[++i];
            else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
        }
        Exec e;
        if (!parse_exec(argv[1], e)) { fprintf(stderr, "exec: operators, fused or pipelined:<1..16>, not '%s'\n", argv[1]); return 2; }
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
            if (e.depth) node.set_depth(e.depth);
            uvo_hip::Published p;
            for (int k = 0; k < n; k++) {
                double meta[2];
                uvo_hip::CompressedMessage m[2];
                if (fread(meta, sizeof(double), 2, f) != 2) { fprintf(stderr, "short frame\n"); return 2; }
                for (int i = 0; i < (stereo ? 2 : 1); i++) if (!read_message(f, m[i])) { fprintf(stderr, "short frame\n"); return 2; }
                if (stereo) node.stereo_imgs_callback(m[0], m[1], meta[0]);
                else { node.range_callback(meta[1]); node.mono_imgs_callback(m[0], meta[0]); }
                for (auto& q : m) std::fill(q.data.begin(), q.data.end(), (unsigned char)0xFF);
                if (e.depth == 0) { write_record(out, node.spin_once()); continue; }
                if (node.in_flight() >= e.depth && node.spin_collect(p)) write_record(out, p);
                if (!node.spin_submit()) throw uvo_hip::Error(UVO_INVALID_ARG, "spin_submit took no frame");
            }
            while (node.spin_collect(p)) write_record(out, p);
            if (fallbacks_path) {
                FILE* d = fopen(fallbacks_path, "w");
                if (!d) { perror("fallbacks"); return 2; }
                fprintf(d, "%d\n", node.compressed_fallbacks()); fclose(d);
            }
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
