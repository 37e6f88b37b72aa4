// flat_normal.hpp — the world normal of a plane node, which depends on the node alone and never on the hit: host only.
// A plane's object-space normal is (0, 1, 0) everywhere (plane.rs), so normal_to_world (object.rs:129-138) gives one
// vector per node.  flatten_scene computes it once per plane (HostScene.flat_normal, uploaded behind DevScene.nodes)
// and the gated kernels read it instead of running the matrix product, the square root and the quotients per pixel
// (device_core.inc prepare_uniform).
// The entry is the reference's value: the full row products of every level's inverse, one normalize per level (a
// correctly rounded sqrt and IEEE quotients), the node's own level first and then its ancestors, compiled without
// contraction like every host unit.  The device forms the same vector with two shortcuts of its own
// (device_core.inc): normal_level drops the off-diagonal products of an NF_DIAG level, which can change the sign of a
// zero component, and div3 replaces the quotients by a reciprocal and a correction, equal to the IEEE quotient over a
// stated range.  flat_plane_normal evaluates that sequence too and reports whether it gives the entry's bits: only
// then may a kernel read the entry in place of its own arithmetic (the fourth value of the table's record), so a
// frame never depends on which of the two it took.
// No HIP and no library state: Node is any record with DevNode's inv, flags and parent (rr_device.hpp), so a native
// check compiles this header alone.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace rr {

constexpr int32_t FN_DIAG = 4;        // == NF_DIAG (flatten.cpp asserts it)
constexpr int32_t FN_TRI_INLINE = 8;  // == NF_TRI_INLINE
constexpr int FLAT_NORMAL_STRIDE = 4;  // doubles per node in the table: x, y, z, usable (1.0 / 0.0)

// one level of normal_to_world as the reference forms it: inverse().transpose() * n, normalized (tuple.rs:95-98)
template <class Node>
inline void flat_normal_level_ref(const Node& nd, double n[3]) {
    const double x = nd.inv[0] * n[0] + nd.inv[4] * n[1] + nd.inv[8] * n[2];
    const double y = nd.inv[1] * n[0] + nd.inv[5] * n[1] + nd.inv[9] * n[2];
    const double z = nd.inv[2] * n[0] + nd.inv[6] * n[1] + nd.inv[10] * n[2];
    const double m = std::sqrt(x * x + y * y + z * z);
    n[0] = x / m;
    n[1] = y / m;
    n[2] = z / m;
}

inline double flat_div_y(double n, double d, double y) {  // device_core.inc div_y
    const double q0 = n * y;
    return std::fma(-std::fma(d, q0, -n), y, q0);
}
// the same level as the device forms it (device_core.inc normal_level, normalize3, div3)
template <class Node>
inline void flat_normal_level_dev(const Node& nd, double n[3]) {
    double x, y, z;
    if (nd.flags & FN_TRI_INLINE) {  // identity inverse (the slots hold a triangle): the same products
        const double I[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
        x = I[0] * n[0] + I[4] * n[1] + I[8] * n[2];
        y = I[1] * n[0] + I[5] * n[1] + I[9] * n[2];
        z = I[2] * n[0] + I[6] * n[1] + I[10] * n[2];
    } else if (nd.flags & FN_DIAG) {
        x = nd.inv[0] * n[0];
        y = nd.inv[5] * n[1];
        z = nd.inv[10] * n[2];
    } else {
        x = nd.inv[0] * n[0] + nd.inv[4] * n[1] + nd.inv[8] * n[2];
        y = nd.inv[1] * n[0] + nd.inv[5] * n[1] + nd.inv[9] * n[2];
        z = nd.inv[2] * n[0] + nd.inv[6] * n[1] + nd.inv[10] * n[2];
    }
    const double m = std::sqrt(x * x + y * y + z * z);
    const double r = 1.0 / m;
    n[0] = flat_div_y(x, m, r);
    n[1] = flat_div_y(y, m, r);
    n[2] = flat_div_y(z, m, r);
}

// out = normal_to_world(nodes[i], (0, 1, 0)), the reference's value.  Returns whether the device's own sequence gives
// exactly these bits (signs of zeros included), i.e. whether a kernel may read `out` in place of computing it.
template <class Node>
inline bool flat_plane_normal(const Node* nodes, int32_t i, double out[3]) {
    double ref[3] = {0.0, 1.0, 0.0}, dev[3] = {0.0, 1.0, 0.0};
    for (int32_t cur = i; cur >= 0; cur = nodes[cur].parent) {
        flat_normal_level_ref(nodes[cur], ref);
        flat_normal_level_dev(nodes[cur], dev);
    }
    out[0] = ref[0];
    out[1] = ref[1];
    out[2] = ref[2];
    return std::memcmp(ref, dev, sizeof(ref)) == 0;
}

}  // namespace rr
