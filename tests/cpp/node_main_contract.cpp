// node_main_contract.cpp -- what the node bootstrap of a catkin workspace asks of ergo_uvo_amd/ros/visual_odometry.h when that
// workspace keeps its own main() (the reference's uvo/src/UVO_node.cpp) and only puts this repository's header first on the include
// path: the header is found as <visual_odometry.h>, std::string is reachable unqualified at file scope (the header's
// `using namespace std`), `visual_odometry_node` is default-constructible and `visual_odometry_workflow` takes that string.
// tests/test_node.py compiles it with -fsyntax-only against tests/cpp/ros_stub/ (not ROS).
#include <visual_odometry.h>

string selected_node;                                   // unqualified on purpose

static void spin_workflow(visual_odometry_node& vo, ros::Rate& rate)
{
    while (ros::ok()) {
        ros::spinOnce();
        rate.sleep();
        ros::param::get("/visual_odometry_node", selected_node);
        vo.visual_odometry_workflow(selected_node);
    }
}

int main(int argc, char** argv)
{
    ros::init(argc, argv, "UVO_node");
    ros::NodeHandle handle;
    ros::Rate rate(20);
    visual_odometry_node vo;
    spin_workflow(vo, rate);
    return 0;
}
