// Recording stand-in for <ros/ros.h> (tests/stubs/README.md): with it in front of tests/stubs/ on the include
// path, ros/geometric_mapping_node.cpp compiles, links against libgm_hip.so and RUNS without ROS.
//   parameters  getParam serves "name value" lines of the text file $GM_ROS_PARAMS; an absent key returns false
//   publishing  advertise and publish append binary records to $GM_ROS_PUBLOG, in order, with every field of the message
//   script      ros::spin() plays $GM_ROS_SCRIPT: messages to the subscribed callback, timer firings, sleeps; then returns
//   logging     ROS_INFO / WARN / ERROR / FATAL append "LEVEL text" lines to $GM_ROS_LOG
//   time        ros::Time::now() is 1234567.000000890, always
// Nothing runs on a clock: createTimer only stores the callback, the script says when it fires.  All integers and floats
// in the two binary files are little-endian as the host stores them; a string is a u32 length and its bytes
// (tests/ros_recorder.py writes the script and reads the log).  Written for this repository; not a copy of roscpp.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <functional>
#include <memory>
#include <string>
#include <vector>
#include <boost_stub_shared_ptr.h>

namespace sensor_msgs { struct PointCloud2; }
namespace visualization_msgs { struct Marker; struct MarkerArray; }

namespace ros {
struct Time { uint32_t sec = 0, nsec = 0; static Time now() { Time t; t.sec = 1234567u; t.nsec = 890u; return t; } };
struct Duration { explicit Duration(double) {} };
struct TimerEvent {};

namespace recorder {

template <class M> struct Kind;   // which record a message type is written as
template <> struct Kind<sensor_msgs::PointCloud2> { enum { value = 1 }; static const char *name() { return "sensor_msgs/PointCloud2"; } };
template <> struct Kind<visualization_msgs::Marker> { enum { value = 2 }; static const char *name() { return "visualization_msgs/Marker"; } };
template <> struct Kind<visualization_msgs::MarkerArray> { enum { value = 3 }; static const char *name() { return "visualization_msgs/MarkerArray"; } };
template <int K> struct Tag {};

class Writer {   // appends to a file; every record is flushed, so the log is whole up to the last publish if the node dies
public:
    explicit Writer(const char *env) : f_(0) { const char *p = std::getenv(env); if (p && *p) f_ = std::fopen(p, "ab"); }
    ~Writer() { if (f_) std::fclose(f_); }
    void bytes(const void *p, size_t n) { if (f_ && n) std::fwrite(p, 1, n, f_); }
    void u8(uint8_t v) { bytes(&v, 1); }
    void u32(uint32_t v) { bytes(&v, 4); }
    void i32(int32_t v) { bytes(&v, 4); }
    void u64(uint64_t v) { bytes(&v, 8); }
    void f32(float v) { bytes(&v, 4); }
    void f64(double v) { bytes(&v, 8); }
    void str(const std::string &s) { u32((uint32_t)s.size()); bytes(s.data(), s.size()); }
    void flush() { if (f_) std::fflush(f_); }
private:
    FILE *f_;
    Writer(const Writer &);
    Writer &operator=(const Writer &);
};

class Reader {   // the script, read whole
public:
    explicit Reader(const char *env) : pos_(0)
    {
        const char *p = std::getenv(env);
        FILE *f = p && *p ? std::fopen(p, "rb") : 0;
        if (!f) return;
        unsigned char chunk[1 << 16];
        for (size_t n; (n = std::fread(chunk, 1, sizeof(chunk), f)) > 0;) buf_.insert(buf_.end(), chunk, chunk + n);
        std::fclose(f);
    }
    bool more() const { return pos_ < buf_.size(); }
    const unsigned char *take(size_t n)
    {
        if (n > buf_.size() - pos_) { std::fprintf(stderr, "ros_recorder: the script ends inside a record\n"); std::exit(97); }
        const unsigned char *p = buf_.data() + pos_;
        pos_ += n;
        return p;
    }
    void unread(size_t n) { pos_ -= n; }
    uint8_t u8() { return *take(1); }
    uint32_t u32() { uint32_t v; std::memcpy(&v, take(4), 4); return v; }
    uint64_t u64() { uint64_t v; std::memcpy(&v, take(8), 8); return v; }
    std::string str() { const uint32_t n = u32(); const unsigned char *p = take(n); return std::string((const char *)p, n); }
private:
    std::vector<unsigned char> buf_;
    size_t pos_;
};

struct State {
    Writer pub, log;
    std::vector<std::pair<std::string, std::string> > params;
    std::function<void(Reader &)> deliver;          // the subscribed callback, fed from a script record
    void (*timer)(const TimerEvent &);
    State() : pub("GM_ROS_PUBLOG"), log("GM_ROS_LOG"), timer(0)
    {
        const char *p = std::getenv("GM_ROS_PARAMS");
        FILE *f = p && *p ? std::fopen(p, "r") : 0;
        if (!f) return;
        char line[1024];
        while (std::fgets(line, sizeof(line), f)) {
            std::string s(line);
            while (!s.empty() && (s[s.size() - 1] == '\n' || s[s.size() - 1] == '\r')) s.erase(s.size() - 1);
            const size_t sp = s.find(' ');
            if (s.empty() || sp == std::string::npos) continue;
            params.push_back(std::make_pair(s.substr(0, sp), s.substr(sp + 1)));
        }
        std::fclose(f);
    }
    const std::string *param(const std::string &name) const
    {
        for (size_t i = 0; i < params.size(); ++i) if (params[i].first == name) return &params[i].second;
        return 0;
    }
};
inline State &state() { static State s; return s; }

inline void console(const char *level, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
inline void console(const char *level, const char *fmt, ...)
{
    char text[2048];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(text, sizeof(text), fmt, ap);
    va_end(ap);
    for (char *c = text; *c; ++c) if (*c == '\n') *c = ' ';   // one line per call
    Writer &w = state().log;
    w.bytes(level, std::strlen(level)); w.bytes(" ", 1); w.bytes(text, std::strlen(text)); w.bytes("\n", 1);
    w.flush();
}

// ---- a message's fields, in the order of its definition.  Templates: the message structs are defined after this header.
template <class H> void put_header(Writer &w, const H &h) { w.u32(h.seq); w.u32(h.stamp.sec); w.u32(h.stamp.nsec); w.str(h.frame_id); }

template <class M> void put(Writer &w, const M &m, Tag<1>)
{
    put_header(w, m.header);
    w.u32(m.height); w.u32(m.width);
    w.u32((uint32_t)m.fields.size());
    for (size_t i = 0; i < m.fields.size(); ++i) {
        w.str(m.fields[i].name); w.u32(m.fields[i].offset); w.u8(m.fields[i].datatype); w.u32(m.fields[i].count);
    }
    w.u8(m.is_bigendian ? 1 : 0); w.u32(m.point_step); w.u32(m.row_step); w.u8(m.is_dense ? 1 : 0);
    w.u64((uint64_t)m.data.size());
    if (!m.data.empty()) w.bytes(&m.data[0], m.data.size());
}

template <class M> void put(Writer &w, const M &m, Tag<2>)
{
    put_header(w, m.header);
    w.str(m.ns); w.i32(m.id); w.i32(m.type); w.i32(m.action);
    w.f64(m.pose.position.x); w.f64(m.pose.position.y); w.f64(m.pose.position.z);
    w.f64(m.pose.orientation.x); w.f64(m.pose.orientation.y); w.f64(m.pose.orientation.z); w.f64(m.pose.orientation.w);
    w.f64(m.scale.x); w.f64(m.scale.y); w.f64(m.scale.z);
    w.f32(m.color.r); w.f32(m.color.g); w.f32(m.color.b); w.f32(m.color.a);
    w.u32((uint32_t)m.points.size());
    for (size_t i = 0; i < m.points.size(); ++i) { w.f64(m.points[i].x); w.f64(m.points[i].y); w.f64(m.points[i].z); }
}

template <class M> void put(Writer &w, const M &m, Tag<3>)
{
    w.u32((uint32_t)m.markers.size());
    for (size_t i = 0; i < m.markers.size(); ++i) put(w, m.markers[i], Tag<2>());
}

// a script's message record into a PointCloud2 (the same fields, the same order)
template <class M> void get_cloud(Reader &r, M &m)
{
    m.header.seq = r.u32(); m.header.stamp.sec = r.u32(); m.header.stamp.nsec = r.u32(); m.header.frame_id = r.str();
    m.height = r.u32(); m.width = r.u32();
    m.fields.resize(r.u32());
    for (size_t i = 0; i < m.fields.size(); ++i) {
        m.fields[i].name = r.str(); m.fields[i].offset = r.u32(); m.fields[i].datatype = r.u8(); m.fields[i].count = r.u32();
    }
    m.is_bigendian = r.u8() != 0; m.point_step = r.u32(); m.row_step = r.u32(); m.is_dense = r.u8() != 0;
    const uint64_t n = r.u64();
    const unsigned char *p = r.take((size_t)n);
    m.data.assign(p, p + n);
}

}  // namespace recorder

class Publisher {
public:
    Publisher() : advertised_(false) {}
    Publisher(const std::string &topic) : topic_(topic), advertised_(true) {}
    // record 'P': topic, advertised (0: this publisher never came from advertise), kind, the message
    template <class M> void publish(const M &m) const
    {
        recorder::Writer &w = recorder::state().pub;
        w.u8('P'); w.str(topic_); w.u8(advertised_ ? 1 : 0); w.u8((uint8_t)recorder::Kind<M>::value);
        recorder::put(w, m, recorder::Tag<recorder::Kind<M>::value>());
        w.flush();
    }
private:
    std::string topic_;
    bool advertised_;
};
class Subscriber { public: ~Subscriber() {} };   // (handles with a destructor, as roscpp's are: holding one is a use)
class Timer { public: ~Timer() {} };

class NodeHandle {
public:
    bool getParam(const std::string &name, double &v) const
    {
        const std::string *s = recorder::state().param(name);
        if (s) v = std::strtod(s->c_str(), 0);
        return s != 0;
    }
    bool getParam(const std::string &name, bool &v) const
    {
        const std::string *s = recorder::state().param(name);
        if (s) v = *s == "true" || *s == "1";
        return s != 0;
    }
    bool getParam(const std::string &name, std::string &v) const
    {
        const std::string *s = recorder::state().param(name);
        if (s) v = *s;
        return s != 0;
    }
    // record 'A': topic, message type, queue size
    template <class M> Publisher advertise(const std::string &topic, uint32_t queue)
    {
        recorder::Writer &w = recorder::state().pub;
        w.u8('A'); w.str(topic); w.str(recorder::Kind<M>::name()); w.u32(queue);
        w.flush();
        return Publisher(topic);
    }
    Timer createTimer(Duration, void (*cb)(const TimerEvent &)) { recorder::state().timer = cb; return Timer(); }
    template <class M> Subscriber subscribe(const std::string &, uint32_t, void (*cb)(const gm_stub::shared_ptr<M const> &))
    {
        recorder::state().deliver = [cb](recorder::Reader &r) {
            std::shared_ptr<M> m(new M());
            recorder::get_cloud(r, *m);
            const gm_stub::shared_ptr<M const> c(m);
            cb(c);
        };
        return Subscriber();
    }
};

inline void init(int &, char **, const std::string &) {}

// Plays the script: 'M' a message for the callback, 'T' u32 k: the timer fires k times, 'S' u32 m: sleep m milliseconds.
// The publish log gets 'C' u32 seq when a callback starts and 'c' when it has returned, 'T' per timer firing and 'E' when
// the script is over, so that a reader can tell which call published what.
inline void spin()
{
    recorder::State &st = recorder::state();
    recorder::Reader script("GM_ROS_SCRIPT");
    while (script.more()) {
        const uint8_t kind = script.u8();
        if (kind == 'M') {
            if (!st.deliver) { std::fprintf(stderr, "ros_recorder: a message, but nothing is subscribed\n"); std::exit(97); }
            const uint32_t seq = script.u32();   // (a look ahead at the header's seq, for the log)
            script.unread(4);
            st.pub.u8('C'); st.pub.u32(seq); st.pub.flush();
            st.deliver(script);
            st.pub.u8('c'); st.pub.flush();
        } else if (kind == 'T') {
            const uint32_t k = script.u32();
            for (uint32_t i = 0; i < k; ++i) {
                st.pub.u8('T'); st.pub.flush();
                if (st.timer) st.timer(TimerEvent());
            }
        } else if (kind == 'S') {
            const uint32_t ms = script.u32();
            struct timespec ts;
            ts.tv_sec = ms / 1000u; ts.tv_nsec = (long)(ms % 1000u) * 1000000L;
            nanosleep(&ts, 0);
        } else {
            std::fprintf(stderr, "ros_recorder: unknown script record %u\n", (unsigned)kind);
            std::exit(97);
        }
    }
    st.pub.u8('E'); st.pub.flush();
}
}  // namespace ros

#define ROS_INFO(...) ::ros::recorder::console("INFO", __VA_ARGS__)
#define ROS_WARN(...) ::ros::recorder::console("WARN", __VA_ARGS__)
#define ROS_ERROR(...) ::ros::recorder::console("ERROR", __VA_ARGS__)
#define ROS_FATAL(...) ::ros::recorder::console("FATAL", __VA_ARGS__)
