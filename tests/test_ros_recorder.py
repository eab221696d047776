"""The recording ROS stand-in checks itself (no GPU): tests/ros_recorder/echo_node.cpp, built against
tests/ros_recorder/ros/ros.h and the message structs of tests/stubs/, is driven by tests/ros_recorder.py.  Parameters,
script records, the publish log and the console log make the round trip unchanged."""
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ros_recorder as rr  # noqa: E402


def test_echo_node_round_trip(tmp_path, monkeypatch):
    exe = str(tmp_path / "echo_node")
    tests = os.path.join(rr.ROOT, "tests")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(tests, "ros_recorder"), "-I",
                    os.path.join(tests, "stubs"), os.path.join(tests, "ros_recorder", "echo_node.cpp"), "-o", exe],
                   check=True, capture_output=True)
    monkeypatch.setattr(rr, "EXE", exe)
    rng = np.random.default_rng(0)
    m1 = rr.message(rng.integers(0, 256, 3 * 2 * 40, dtype=np.uint8), 2, height=3, point_step=19, row_step=40, seq=4000000001,
                    stamp=(17, 999999999), frame_id="a frame", bigendian=True, dense=False,
                    fields=[("x", 1, rr.FLOAT32, 1), ("tag", 5, 2, 3), ("", 0, rr.FLOAT64, 0)])
    m2 = rr.message(np.zeros(0, np.uint8), 0, fields=[], frame_id="")
    r = rr.run(dict(aDouble=0.1, aBool=True, aString="0,0 and more"),
               [("msg", m1), ("timer", 2), ("sleep", 3), ("msg", m2)], timeout=30)
    assert r.log == [("WARN", "1 1 1 0 0.10000000000000001 1 0,0 and more"), ("INFO", "got 3 x 2"), ("INFO", "got 1 x 0"),
                     ("ERROR", "done")]
    assert r.advertised() == [("echo", "sensor_msgs/PointCloud2", 7), ("marker", "visualization_msgs/Marker", 1),
                              ("array", "visualization_msgs/MarkerArray", 2)]
    ev = [e["ev"] + (":" + e["topic"] if e["ev"] == "publish" else "") for e in r.events if e["ev"] != "advertise"]
    assert ev == ["callback", "publish:echo", "callback_end", "timer", "publish:marker", "publish:array", "timer",
                  "publish:marker", "publish:array", "callback", "publish:echo", "callback_end", "spin_end", "publish:"]
    assert [e["seq"] for e in r.events if e["ev"] == "callback"] == [4000000001, 0]
    for sent, got in zip((m1, m2), r.published("echo")):
        g = got["msg"]
        assert got["advertised"] and got["kind"] == "cloud"
        assert g["header"] == dict(seq=sent["seq"], stamp=sent["stamp"], frame_id=sent["frame_id"])
        for k in ("height", "width", "fields", "is_bigendian", "point_step", "row_step", "is_dense"):
            assert g[k] == sent[k], k
        assert np.array_equal(g["data"], sent["data"])
    mk = r.published("marker")[1]["msg"]
    assert mk["header"] == dict(seq=3, stamp=rr.NOW, frame_id="/f")
    assert (mk["ns"], mk["id"], mk["type"], mk["action"]) == ("ns", -2, 3, 0)
    assert mk["position"].tolist() == [1.5, -2.5, 3.5] and mk["orientation"].tolist() == [0.1, 0.2, 0.3, 0.4]
    assert mk["scale"].tolist() == [4.0, 5.0, 6.0] and mk["points"].tolist() == [[0.0, 0.0, 0.0], [7.0, 8.0, 9.0]]
    assert {k: float(v) for k, v in mk["color"].items()} == dict(r=0.25, g=0.5, b=0.75, a=1.0)
    arr = r.published("array")[0]["msg"]
    assert [a["id"] for a in arr] == [-2, 5] and arr[1]["points"].tolist() == mk["points"].tolist()
    stray = r.published("")[0]
    assert stray["advertised"] is False and stray["kind"] == "markers" and stray["msg"] == []
