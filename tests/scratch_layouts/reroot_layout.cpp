// Test infrastructure of tests/test_reroot_scratch_layout.py: what rrtplanner_amd/csrc/rrt_scratch.h makes of the scratch layout of the
// reroot call (RerootScratch), printed and used the way scratch_layouts.cpp does for the other layouts.  It includes that header alone
// and is compiled with
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
    RerootScratch l;
    explicit Probe(size_t cap) : block(static_cast<unsigned char *>(std::malloc(RerootScratch(nullptr, cap).bytes))), l(block, cap) {
        const RerootScratch counted(nullptr, cap);
        if (!block || counted.bytes != l.bytes) std::abort();
        std::printf("layout reroot_tmp %zu %zu\n", cap, counted.bytes);
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
        p.array("out_vcost", p.l.out_vcost, cap);
        p.array("out_nodes", p.l.out_nodes, cap);
        p.array("out_parent", p.l.out_parent, cap);
        p.array("out_id", p.l.out_id, cap);
        p.array("path", p.l.path, cap);
        p.array("new_parent", p.l.new_parent, cap);
        p.array("anc0", p.l.anc[0], cap);
        p.array("anc1", p.l.anc[1], cap);
        p.array("dep0", p.l.dep[0], cap);
        p.array("dep1", p.l.dep[1], cap);
        p.array("level_cnt", p.l.level_cnt, cap + 1);
        p.array("level_start", p.l.level_start, cap + 1);
        p.array("rank", p.l.rank, cap);
        p.array("src", p.l.src, cap);
        p.array("head", p.l.head, 8);
        p.array("ok0", p.l.ok[0], cap8);
        p.array("ok1", p.l.ok[1], cap8);
    }
    return 0;
}
