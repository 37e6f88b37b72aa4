// flat_normal_check.cpp — the per-node table of planes' world normals (rray_amd/csrc/flat_normal.hpp, the header
// flatten.cpp fills the table behind DevScene.nodes with) on the host.  Reads cases from the file named on the command line, one
// per line: the number of levels L (the plane, then its group ancestors, innermost first), then per level the 12
// entries of rows 0..2 of its inverse as hex doubles.  Each level gets the flags flatten_scene gives it (identity:
// NF_IDENT; diagonal + translation: NF_DIAG).  Prints per case the table entry as three hex doubles, the plane's flags,
// whether the kernels may read the entry (their own sequence gives its bits), and that sequence's own three values.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "flat_normal.hpp"

struct Node {  // the fields of DevNode the header reads
    double inv[12];
    int32_t flags;
    int32_t parent;
};

static bool is_diag12(const double* m) {
    return m[1] == 0.0 && m[2] == 0.0 && m[4] == 0.0 && m[6] == 0.0 && m[8] == 0.0 && m[9] == 0.0;
}
static bool is_identity12(const double* m) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c)
            if (m[r * 4 + c] != (r == c ? 1.0 : 0.0)) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int L;
    while (std::fscanf(f, "%d", &L) == 1) {
        if (L < 1 || L > 8) return 3;
        std::vector<Node> nodes((size_t)L);
        for (int l = 0; l < L; ++l) {
            for (int k = 0; k < 12; ++k)
                if (std::fscanf(f, "%la", &nodes[l].inv[k]) != 1) return 3;
            nodes[l].flags = is_identity12(nodes[l].inv) ? 1 : is_diag12(nodes[l].inv) ? rr::FN_DIAG : 0;
            nodes[l].parent = l + 1 < L ? l + 1 : -1;
        }
        double n[3], dev[3] = {0.0, 1.0, 0.0};
        const bool usable = rr::flat_plane_normal(nodes.data(), 0, n);
        for (int l = 0; l < L; ++l) rr::flat_normal_level_dev(nodes[l], dev);
        std::printf("%a %a %a %d %d %a %a %a\n", n[0], n[1], n[2], nodes[0].flags, usable ? 1 : 0, dev[0], dev[1], dev[2]);
    }
    std::fclose(f);
    return 0;
}
