// Test infrastructure of tests/test_pose_reroot_scratch_layout.py: what rrtplanner_amd/csrc/rrt_scratch.h makes of the scratch layout of the
// reroot_poses call (PoseRerootScratch), printed and used the way pose_relax_layout.cpp does for PoseRelaxScratch.  It includes that
// header alone and is compiled with
//     g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined
// Per capacity: the bytes counted over a null base; then a heap block of exactly that many bytes is carved and the first and last
// element of every array written, so that an array that runs past the bytes is the sanitizer's to report.  The lengths of the arrays
// are stated here, independently of the header.  Output, one line each:
//     layout <name> <cap> <bytes>
//     array <name> <offset> <element size> <length>
#include "rrt_scratch.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

struct Probe {
    unsigned char *block;
    PoseRerootScratch l;
    explicit Probe(size_t cap) : block(static_cast<unsigned char *>(std::malloc(PoseRerootScratch(nullptr, cap).bytes))), l(block, cap) {
        const PoseRerootScratch counted(nullptr, cap);
        if (!block || counted.bytes != l.bytes) std::abort();
        std::printf("layout pose_reroot_tmp %zu %zu\n", cap, counted.bytes);
    }
    ~Probe() { std::free(block); }
    template <typename T>
    void array(const char *name, T *p, size_t count) const {
        std::printf("array %s %td %zu %zu\n", name, reinterpret_cast<unsigned char *>(p) - block, sizeof(T), count);
        p[0] = T(1);
        p[count - 1] = T(2);
    }
};

int main() {
    for (size_t cap : {1, 2, 7, 8, 9, 255, 256, 257, 4097}) {
        const size_t cap8 = (cap + 7) / 8 * 8;
        Probe p(cap);
        p.array("f_nodes", p.l.f_nodes, cap);
        p.array("f_parent", p.l.f_parent, cap);
        p.array("f_id", p.l.f_id, cap);
        p.array("f_heading", p.l.f_heading, cap8);
    }
    return 0;
}
