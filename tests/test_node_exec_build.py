"""The execution-mode driver and the ROS adapter's `~execution` meet a compiler without a GPU: the shim Makefile builds
tests/cpp/shim_vo_node_exec, its --config-only is shim_vo_node's, and the adapter header still passes the stub-header syntax check."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_node as TN

DRIVER = os.path.join(TN.ROOT, "tests", "cpp", "build", "shim_vo_node_exec")


def test_shim_makefile_builds_the_exec_driver():
    TN._build()
    assert os.access(DRIVER, os.X_OK)
    res = subprocess.run([DRIVER, "warp", "stereo", "cam", "a", "b", "c", "d"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "operators, fused or pipelined" in res.stderr            # the mode is parsed before any file or the GPU is touched


def test_exec_driver_config_only_is_the_node_drivers(tmp_path):
    TN._build()
    for mode, texts in (("mono", (TN.MONO_PARAMS, TN.MONO_INTRINSICS)), ("stereo", (TN.STEREO_PARAMS, TN.STEREO_INTRINSICS))):
        files = []
        for i, t in enumerate(texts):
            p = tmp_path / f"{mode}{i}.yaml"; p.write_text(t); files.append(str(p))
        outs = [subprocess.run([exe, "--config-only", mode, "frontal_camera"] + files, capture_output=True, text=True, timeout=120) for exe in (TN.DRIVER, DRIVER)]
        assert outs[0].returncode == 0 and outs[1].returncode == 0, (outs[0].stderr, outs[1].stderr)
        assert outs[1].stdout == outs[0].stdout and "PNP_METHOD_FLAG" in outs[1].stdout


def test_ros_adapter_with_execution_parameter_meets_a_compiler():
    """the command of test_node.test_ros_adapter_meets_a_compiler, and the header does read `~execution` and hand it to the node class"""
    ros_dir = os.path.join(TN.ROOT, "ergo_uvo_amd", "ros")
    hdr = open(os.path.join(ros_dir, "visual_odometry.h")).read()
    assert '"~execution"' in hdr and "CAMERA_NAME, execution)" in hdr
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-DUVO_NO_OPENCV", "-Wall", "-Wextra", "-Wno-unused-variable", "-Wno-unused-but-set-variable",
           "-I", ros_dir, "-I", os.path.join(TN.ROOT, "include"), "-I", os.path.join(TN.ROOT, "tests", "cpp", "ros_stub"), os.path.join(ros_dir, "UVO_node_hip.cpp")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    # the check bites on the new code: the device-resident callback misspelt does not compile
    bad = hdr.replace("core->mono_imgs_callback(from_ros_to_device_image(msg)", "core->mono_imgs_calback(from_ros_to_device_image(msg)") + "\nint main() { visual_odometry_node n; n.visual_odometry_workflow(\"mono\"); }\n"
    assert bad != hdr
    res = subprocess.run(cmd[:-1] + ["-x", "c++", "-"], input=bad, capture_output=True, text=True, timeout=120, cwd=ros_dir)
    assert res.returncode != 0 and "mono_imgs_calback" in res.stderr
