"""The compressed-message driver and the ROS adapter's hand-over meet a compiler without a GPU: the shim Makefile builds
tests/cpp/shim_vo_node_compressed, its --config-only is shim_vo_node's, and the adapter header, which now hands the message on to the
node class instead of decoding in the callback, still passes the stub-header syntax check."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_node as TN

DRIVER = os.path.join(TN.ROOT, "tests", "cpp", "build", "shim_vo_node_compressed")


def test_shim_makefile_builds_the_compressed_driver():
    TN._build()
    assert os.access(DRIVER, os.X_OK)
    res = subprocess.run([DRIVER, "warp", "stereo", "cam", "a", "b", "c", "d"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "operators, fused or pipelined" in res.stderr            # the mode is parsed before any file or the GPU is touched


def test_compressed_driver_config_only_is_the_node_drivers(tmp_path):
    TN._build()
    files = []
    for i, t in enumerate((TN.STEREO_PARAMS, TN.STEREO_INTRINSICS)):
        p = tmp_path / f"stereo{i}.yaml"; p.write_text(t); files.append(str(p))
    outs = [subprocess.run([exe, "--config-only", "stereo", "frontal_camera"] + files, capture_output=True, text=True, timeout=120) for exe in (TN.DRIVER, DRIVER)]
    assert outs[0].returncode == 0 and outs[1].returncode == 0, (outs[0].stderr, outs[1].stderr)
    assert outs[1].stdout == outs[0].stdout


def test_ros_adapter_hands_the_message_on_and_meets_a_compiler():
    ros_dir = os.path.join(TN.ROOT, "ergo_uvo_amd", "ros")
    hdr = open(os.path.join(ros_dir, "visual_odometry.h")).read()
    assert '"~ingest"' in hdr and "core->stereo_imgs_callback(from_ros_to_message(left_image), from_ros_to_message(right_image)" in hdr
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-DUVO_NO_OPENCV", "-Wall", "-Wextra", "-Wno-unused-variable", "-Wno-unused-but-set-variable",
           "-I", ros_dir, "-I", os.path.join(TN.ROOT, "include"), "-I", os.path.join(TN.ROOT, "tests", "cpp", "ros_stub"), os.path.join(ros_dir, "UVO_node_hip.cpp")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    # the check bites on the new code: the hand-over with a member of the message misspelt does not compile
    bad = hdr.replace("m.format = msg->format;", "m.format = msg->fromat;") + "\nint main() { visual_odometry_node n; n.visual_odometry_workflow(\"mono\"); }\n"
    assert bad != hdr
    res = subprocess.run(cmd[:-1] + ["-x", "c++", "-"], input=bad, capture_output=True, text=True, timeout=120, cwd=ros_dir)
    assert res.returncode != 0 and "fromat" in res.stderr
