// shim_vo_node_akaze.cpp -- test driver: the node class on raw frames in one execution mode, with AKAZE::create's arguments handed to the
// mirror (uvo_hip::configure_akaze) BEFORE the node is made -- the parameter files have no AKAZE keys, so this call is how a node gets them.
//
//   usage: shim_vo_node_akaze <akaze> <exec> <mono|stereo> <camera_name> <frames.bin> <out.bin> <params.yaml> <intrinsics.yaml>
//   akaze     : default (configure_akaze is not called) | descriptor_type,descriptor_size,descriptor_channels,threshold,nOctaves,nOctaveLayers,diffusivity
//   exec      : operators | fused | pipelined:<depth>
//   frames.bin, out.bin: as shim_vo_node_exec (one record per frame, in the order of the frames)
#include <string>

#define main shim_vo_node_main             // the existing driver's read_rgb(), not its main()
#include "shim_vo_node.cpp"
#undef main

namespace {

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
        if (argc != 9) { fprintf(stderr, "usage: %s default|t,s,c,threshold,octaves,layers,diffusivity operators|fused|pipelined:<depth> mono|stereo camera frames.bin out.bin params.yaml intrinsics.yaml\n", argv[0]); return 2; }
        if (strcmp(argv[1], "default") != 0) {
            int t, s, c, o, l, d; float thr;
            if (sscanf(argv[1], "%d,%d,%d,%f,%d,%d,%d", &t, &s, &c, &thr, &o, &l, &d) != 7) { fprintf(stderr, "akaze: default, or seven comma-separated values\n"); return 2; }
            uvo_hip::configure_akaze(t, s, c, thr, o, l, d);
        }
        const std::string ex = argv[2], mode = argv[3];
        int depth = 0;
        if (ex.rfind("pipelined:", 0) == 0) depth = atoi(ex.c_str() + 10);
        else if (ex != "operators" && ex != "fused") { fprintf(stderr, "exec: operators, fused or pipelined:<1..16>\n"); return 2; }
        if (ex.rfind("pipelined:", 0) == 0 && (depth < 1 || depth > 16)) { fprintf(stderr, "exec: pipelined:<1..16>\n"); return 2; }
        const bool stereo = mode == "stereo";
        uvo_hip::ParamTree tree;
        tree.load_yaml_file(argv[7]); tree.load_yaml_file(argv[8]);
        FILE* f = fopen(argv[5], "rb");
        if (!f) { perror("frames"); return 2; }
        int hdr[3];
        if (fread(hdr, sizeof(int), 3, f) != 3) { fprintf(stderr, "short header\n"); return 2; }
        const int W = hdr[0], H = hdr[1], n = hdr[2];
        const int max_kpts = getenv("UVO_TEST_MAX_KPTS") ? atoi(getenv("UVO_TEST_MAX_KPTS")) : 8192;
        uvo_hip::configure(0, W > 640 ? W : 640, H > 480 ? H : 480, max_kpts);       // (rebuilds the context: the AKAZE arguments are kept across it)
        FILE* out = fopen(argv[6], "wb");
        if (!out) { perror("out"); return 2; }
        {
            uvo_hip::visual_odometry_core node(mode, tree, argv[4], ex == "operators" ? uvo_hip::Execution::operators : uvo_hip::Execution::fused);
            if (depth) node.set_depth(depth);
            uvo_hip::Published p;
            for (int k = 0; k < n; k++) {
                double meta[2];
                Mat img[2];                                                 // a new Mat per frame: the node holds a submitted frame's until its collect
                if (fread(meta, sizeof(double), 2, f) != 2) { fprintf(stderr, "short frame\n"); return 2; }
                for (int i = 0; i < (stereo ? 2 : 1); i++) if (!read_rgb(f, W, H, img[i])) { fprintf(stderr, "short frame\n"); return 2; }
                if (stereo) node.stereo_imgs_callback(img[0], img[1], meta[0]);
                else { node.range_callback(meta[1]); node.mono_imgs_callback(img[0], meta[0]); }
                if (depth == 0) { write_record(out, node.spin_once()); continue; }
                if (node.in_flight() >= depth && node.spin_collect(p)) write_record(out, p);
                if (!node.spin_submit()) throw uvo_hip::Error(UVO_INVALID_ARG, "spin_submit took no frame");
            }
            while (depth && node.spin_collect(p)) write_record(out, p);
        }
        fclose(out); fclose(f);
        uvo_hip::shutdown();
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
