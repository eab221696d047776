"""Driver of the recorded ROS node (test infrastructure): host/gm_ros_node_recorded is ros/geometric_mapping_node.cpp
built against tests/ros_recorder/ros/ros.h, which serves parameters from a file, plays a script instead of ros::spin()
and logs everything the node publishes and prints.  This module writes the two input files from numpy arrays, runs the
node as a fresh child process with a timeout, and reads both logs back.  File formats: tests/ros_recorder/ros/ros.h."""
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_ros_node_recorded")
NOW = (1234567, 890)   # ros::Time::now() of the stand-in
FLOAT32, FLOAT64 = 7, 8   # sensor_msgs/PointField datatypes
# launch/mapping.launch:7-15 of the reference
LAUNCH = dict(boxFilterBound=5.0, voxelGridLeafSize=0.5, neighborRadius=0.5, weightingFactor=0.2, displayCloud=True,
              displayNormals=False, displayCenterAxis=True, displayCylinder=False, usePCLViz=False)


_abnormal = []   # set by the first child that ends by a signal or overruns its timeout


def build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_ros_node_recorded"], check=True, capture_output=True)
    return EXE


def _s(text):
    b = text.encode()
    return struct.pack("<I", len(b)) + b


def message(data, width, height=1, point_step=16, row_step=None, fields=None, seq=0, stamp=(0, 0), frame_id="/velodyne",
            bigendian=False, dense=True):
    """One sensor_msgs/PointCloud2 as a dict.  data: uint8 array (any shape); fields: [(name, offset, datatype, count)],
    by default float32 x, y, z at 0, 4, 8."""
    if fields is None:
        fields = [("x", 0, FLOAT32, 1), ("y", 4, FLOAT32, 1), ("z", 8, FLOAT32, 1)]
    return dict(seq=seq, stamp=tuple(stamp), frame_id=frame_id, height=height, width=width, fields=list(fields),
                is_bigendian=bool(bigendian), point_step=point_step,
                row_step=width * point_step if row_step is None else row_step, is_dense=bool(dense),
                data=np.ascontiguousarray(data, dtype=np.uint8).reshape(-1))


def xyz_message(xyz, point_step=16, offsets=(0, 4, 8), fill=0, **kw):
    """(n, 3) float32 points as unorganised rows of point_step bytes, the other bytes `fill`."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    rows = np.full((xyz.shape[0], point_step), fill, dtype=np.uint8)
    raw = xyz.view(np.uint8).reshape(xyz.shape[0], 12)
    for k, off in enumerate(offsets):
        rows[:, off:off + 4] = raw[:, 4 * k:4 * k + 4]
    kw.setdefault("fields", [(name, off, FLOAT32, 1) for name, off in zip("xyz", offsets)])
    return message(rows, xyz.shape[0], point_step=point_step, **kw)


def _message_bytes(m):
    out = [struct.pack("<III", m["seq"], m["stamp"][0], m["stamp"][1]), _s(m["frame_id"]),
           struct.pack("<III", m["height"], m["width"], len(m["fields"]))]
    for name, offset, datatype, count in m["fields"]:
        out += [_s(name), struct.pack("<IBI", offset, datatype, count)]
    out.append(struct.pack("<BIIBQ", m["is_bigendian"], m["point_step"], m["row_step"], m["is_dense"], m["data"].size))
    out.append(m["data"].tobytes())
    return b"".join(out)


def script_bytes(script):
    """script: a list of ("msg", message dict) | ("timer", k) | ("sleep", milliseconds)."""
    out = []
    for kind, arg in script:
        if kind == "msg":
            out.append(b"M" + _message_bytes(arg))
        elif kind == "timer":
            out.append(b"T" + struct.pack("<I", arg))
        elif kind == "sleep":
            out.append(b"S" + struct.pack("<I", arg))
        else:
            raise ValueError(kind)
    return b"".join(out)


def params_text(params):
    lines = []
    for k, v in params.items():
        lines.append("%s %s" % (k, ("true" if v else "false") if isinstance(v, bool) else repr(v) if isinstance(v, float) else v))
    return "\n".join(lines) + "\n"


class _Cursor:
    def __init__(self, buf):
        self.buf, self.pos = buf, 0

    def take(self, fmt):
        v = struct.unpack_from("<" + fmt, self.buf, self.pos)
        self.pos += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def raw(self, n):
        b = self.buf[self.pos:self.pos + n]
        assert len(b) == n, "the publish log ends inside a record"
        self.pos += n
        return b

    def text(self):
        return self.raw(self.take("I")).decode()


def _header(c):
    seq, sec, nsec = c.take("III")
    return dict(seq=seq, stamp=(sec, nsec), frame_id=c.text())


def _cloud(c):
    m = dict(header=_header(c))
    m["height"], m["width"], nf = c.take("III")
    m["fields"] = []
    for _ in range(nf):
        name = c.text()
        m["fields"].append((name,) + tuple(c.take("IBI")))
    m["is_bigendian"], m["point_step"], m["row_step"], m["is_dense"], n = c.take("BIIBQ")
    m["is_bigendian"], m["is_dense"] = bool(m["is_bigendian"]), bool(m["is_dense"])
    m["data"] = np.frombuffer(c.raw(n), dtype=np.uint8)
    return m


def _marker(c):
    m = dict(header=_header(c), ns=c.text())
    m["id"], m["type"], m["action"] = c.take("iii")
    m["position"] = np.array(c.take("3d"))
    m["orientation"] = np.array(c.take("4d"))   # x, y, z, w
    m["scale"] = np.array(c.take("3d"))
    r, g, b, a = np.frombuffer(c.raw(16), dtype=np.float32)
    m["color"] = dict(r=r, g=g, b=b, a=a)
    n = c.take("I")
    m["points"] = np.frombuffer(c.raw(24 * n), dtype=np.float64).reshape(n, 3)
    return m


def read_publog(buf):
    """The publish log as a list of events, in order:
    dict(ev="advertise", topic, type, queue) | dict(ev="publish", topic, advertised, kind="cloud"|"marker"|"markers", msg) |
    dict(ev="callback", seq) | dict(ev="callback_end") | dict(ev="timer") | dict(ev="spin_end")."""
    c, out = _Cursor(buf), []
    while c.pos < len(buf):
        k = chr(c.take("B"))
        if k == "A":
            out.append(dict(ev="advertise", topic=c.text(), type=c.text(), queue=c.take("I")))
        elif k == "P":
            e = dict(ev="publish", topic=c.text(), advertised=bool(c.take("B")))
            kind = c.take("B")
            if kind == 1:
                e["kind"], e["msg"] = "cloud", _cloud(c)
            elif kind == 2:
                e["kind"], e["msg"] = "marker", _marker(c)
            elif kind == 3:
                e["kind"], e["msg"] = "markers", [_marker(c) for _ in range(c.take("I"))]
            else:
                raise ValueError("publish record of kind %d" % kind)
            out.append(e)
        elif k == "C":
            out.append(dict(ev="callback", seq=c.take("I")))
        elif k == "c":
            out.append(dict(ev="callback_end"))
        elif k == "T":
            out.append(dict(ev="timer"))
        elif k == "E":
            out.append(dict(ev="spin_end"))
        else:
            raise ValueError("publish log record %r at byte %d" % (k, c.pos - 1))
    return out


class Run:
    """What one child run left: returncode, events (read_publog), log = [(level, text)], stderr."""

    def __init__(self, returncode, events, log, stderr):
        self.returncode, self.events, self.log, self.stderr = returncode, events, log, stderr

    def published(self, topic=None):
        return [e for e in self.events if e["ev"] == "publish" and (topic is None or e["topic"] == topic)]

    def advertised(self):
        return [(e["topic"], e["type"], e["queue"]) for e in self.events if e["ev"] == "advertise"]

    def lines(self, level=None):
        return [t for lv, t in self.log if level is None or lv == level]

    def report(self):
        return "exit status %s\n--- node log ---\n%s\n--- events ---\n%s\n--- stderr ---\n%s" % (
            self.returncode, "\n".join("%s %s" % lt for lt in self.log),
            " ".join(e["ev"] + (":" + e["topic"] if "topic" in e else "") for e in self.events), self.stderr[-2000:])


def run(params, script, timeout=120, expect_exit=0):
    """Runs the node once on `script` under `params` (a dict; LAUNCH is not implied).  Raises AssertionError with both logs
    when the child ends abnormally (a signal, or an exit status other than expect_exit) or overruns the timeout."""
    assert not _abnormal, "an earlier child run ended abnormally (%s): no further child is started" % _abnormal[0]
    exe = EXE if os.path.exists(EXE) else build()
    with tempfile.TemporaryDirectory() as d:
        paths = {k: os.path.join(d, k) for k in ("params", "script", "publog", "log")}
        with open(paths["params"], "w") as f:
            f.write(params_text(params))
        with open(paths["script"], "wb") as f:
            f.write(script_bytes(script))
        env = dict(os.environ, GM_ROS_PARAMS=paths["params"], GM_ROS_SCRIPT=paths["script"], GM_ROS_PUBLOG=paths["publog"],
                   GM_ROS_LOG=paths["log"])
        try:
            r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=timeout)
            code, err = r.returncode, r.stdout + r.stderr
        except subprocess.TimeoutExpired as e:
            code, err = None, "timed out after %s s\n%s" % (timeout, e.stderr or "")
        pub = open(paths["publog"], "rb").read() if os.path.exists(paths["publog"]) else b""
        text = open(paths["log"], errors="replace").read() if os.path.exists(paths["log"]) else ""
    log = [tuple(line.split(" ", 1)) if " " in line else (line, "") for line in text.splitlines()]
    try:
        events = read_publog(pub)
    except (AssertionError, ValueError, struct.error) as e:   # (a log cut short by a crash)
        events, err = [], err + "\nunreadable publish log: %s" % e
    out = Run(code, events, log, err)
    if code is None or code < 0:   # a time limit or a signal: whatever comes next in this process starts no other child
        _abnormal.append("timeout" if code is None else "signal %d" % -code)
    assert code == expect_exit, out.report()
    return out
