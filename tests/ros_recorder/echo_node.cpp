// The recording stand-in's own check (tests/test_ros_recorder.py, no GPU): a node that reads three parameters, republishes
// every message it receives, publishes one marker and one marker array per timer firing, and publishes once on a topic it
// never advertised.
#include <ros/ros.h>
#include <sensor_msgs/PointCloud2.h>
#include <visualization_msgs/MarkerArray.h>

static ros::Publisher echo, markerPub, arrayPub, stray;

static void cloud_cb(const sensor_msgs::PointCloud2ConstPtr &in)
{
    ROS_INFO("got %u x %u", in->height, in->width);
    echo.publish(*in);
}

static void timer_cb(const ros::TimerEvent &)
{
    visualization_msgs::Marker m;
    m.header.frame_id = "/f"; m.header.stamp = ros::Time::now(); m.header.seq = 3;
    m.ns = "ns"; m.id = -2; m.type = visualization_msgs::Marker::CYLINDER; m.action = visualization_msgs::Marker::ADD;
    m.pose.position.x = 1.5; m.pose.position.y = -2.5; m.pose.position.z = 3.5;
    m.pose.orientation.x = 0.1; m.pose.orientation.y = 0.2; m.pose.orientation.z = 0.3; m.pose.orientation.w = 0.4;
    m.scale.x = 4; m.scale.y = 5; m.scale.z = 6;
    m.color.r = 0.25f; m.color.g = 0.5f; m.color.b = 0.75f; m.color.a = 1.0f;
    m.points.resize(2);
    m.points[1].x = 7; m.points[1].y = 8; m.points[1].z = 9;
    markerPub.publish(m);
    visualization_msgs::MarkerArray a;
    a.markers.assign(2, m);
    a.markers[1].id = 5;
    arrayPub.publish(a);
}

int main(int argc, char **argv)
{
    ros::init(argc, argv, "echo");
    ros::NodeHandle node;
    double d = -1; bool b = false; std::string s = "unset", absent = "unset";
    const bool gd = node.getParam("aDouble", d), gb = node.getParam("aBool", b), gs = node.getParam("aString", s);
    ROS_WARN("%d %d %d %d %.17g %d %s", gd, gb, gs, node.getParam("absent", absent), d, b, s.c_str());
    ros::Subscriber sub = node.subscribe("input", 1, cloud_cb);
    ros::Timer timer = node.createTimer(ros::Duration(0.002), timer_cb);
    echo = node.advertise<sensor_msgs::PointCloud2>("echo", 7);
    markerPub = node.advertise<visualization_msgs::Marker>("marker", 1);
    arrayPub = node.advertise<visualization_msgs::MarkerArray>("array", 2);
    ros::spin();
    stray.publish(visualization_msgs::MarkerArray());
    ROS_ERROR("done");
    return 0;
}
