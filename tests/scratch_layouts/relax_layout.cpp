// Test infrastructure of tests/test_relax_scratch_layout.py: what rrtplanner_amd/csrc/rrt_scratch.h makes of the scratch layout of the
// relax call (RelaxScratch), printed and used the way reroot_layout.cpp does for RerootScratch.  It includes that header alone and is
// compiled with
//     g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined
// Per capacity and cell count: the bytes counted over a null base; then a heap block of exactly that many bytes is carved and the
// first and last element of every array written, so that an array that runs past the bytes is the sanitizer's to report.  The lengths
// of the arrays are stated here, independently of the header.  Output, one line each:
//     layout <name> <cap> <cells> <bytes>
//     array <name> <offset> <element size> <length>
#include "rrt_scratch.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

struct Probe {
    unsigned char *block;
    RelaxScratch l;
    Probe(size_t cap, size_t cells) : block(static_cast<unsigned char *>(std::malloc(RelaxScratch(nullptr, cap, cells).bytes))), l(block, cap, cells) {
        const RelaxScratch counted(nullptr, cap, cells);
        if (!block || counted.bytes != l.bytes) std::abort();
        std::printf("layout relax_tmp %zu %zu %zu\n", cap, cells, counted.bytes);
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
    for (size_t cells : {1, 9, 4096})
        for (size_t cap : {1, 2, 7, 8, 9, 255, 256, 257, 4097}) {
            const size_t cells8 = (cells + 7) / 8 * 8;
            Probe p(cap, cells);
            p.array("cost", p.l.cost, cap);
            p.array("stats", p.l.stats, 4);
            p.array("cell_of", p.l.cell_of, cap);
            p.array("items", p.l.items, cap);
            p.array("item_xy", p.l.item_xy, cap);
            p.array("pos_of", p.l.pos_of, cap);
            p.array("cell_start", p.l.cell_start, cells + 1);
            p.array("cell_fill", p.l.cell_fill, cells);
            p.array("dirty0", p.l.dirty[0], cells8);
            p.array("dirty1", p.l.dirty[1], cells8);
            p.array("changed0", p.l.changed[0], (cap + 7) / 8 * 8);
            p.array("changed1", p.l.changed[1], (cap + 7) / 8 * 8);
        }
    return 0;
}
