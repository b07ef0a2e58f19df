// Test infrastructure of tests/test_scratch_layouts.py: prints what rrtplanner_amd/csrc/rrt_scratch.h makes of every scratch layout
// of the tree calls, and uses every buffer the way the library does.  It includes that header alone and is compiled with
//     g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined
// Per layout and capacity: the bytes counted over a null base; then a heap block of exactly that many bytes is carved and the first
// and last element of every array written, so that an array that runs past the bytes is the sanitizer's to report.  The lengths of
// the arrays are stated here, independently of the header.  Output, one line each:
//     layout <name> <cap> <bytes>
//     array <name> <offset> <element size> <length>
#include "rrt_scratch.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

template <typename Layout, typename... Extra>
struct Probe {
    unsigned char *block;
    Layout l;
    Probe(const char *name, size_t cap, Extra... extra)
        : block(static_cast<unsigned char *>(std::malloc(Layout(nullptr, cap, extra...).bytes))), l(block, cap, extra...) {
        const Layout counted(nullptr, cap, extra...);
        if (!block || counted.bytes != l.bytes) std::abort();
        std::printf("layout %s %zu %zu\n", name, cap, counted.bytes);
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
        {
            Probe<RouteGoalScratch> p("route_goal", cap);
            p.array("length", p.l.length, cap);
            p.array("raw_off", p.l.raw_off, cap + 1);
            p.array("fin_off", p.l.fin_off, cap + 1);
            p.array("cnt", p.l.cnt, cap);
            p.array("kept", p.l.kept, cap);
            p.array("err", p.l.err, 1);
        }
        {
            Probe<RouteRowScratch> p("route_row", cap);
            p.array("row_xy", p.l.row_xy, cap);
            p.array("row_id", p.l.row_id, cap);
            p.array("out_xy", p.l.out_xy, 2 * cap);
            p.array("out_id", p.l.out_id, cap);
        }
        {
            Probe<PoseRouteGoalScratch> p("pose_route_goal", cap);
            p.array("length", p.l.length, cap);
            p.array("raw_off", p.l.raw_off, cap + 1);
            p.array("goal_pt_off", p.l.goal_pt_off, cap + 1);
            p.array("cnt", p.l.cnt, cap);
            p.array("err", p.l.err, 1);
        }
        {
            Probe<PoseRouteRowScratch> p("pose_route_row", cap);
            p.array("leg_len", p.l.leg_len, cap);
            p.array("pt_off", p.l.pt_off, cap + 1);
            p.array("row_xy", p.l.row_xy, cap);
            p.array("row_id", p.l.row_id, cap);
            p.array("npts", p.l.npts, cap);
            p.array("row_h", p.l.row_h, cap);
        }
        {
            Probe<PoseCutGoalScratch> p("pose_cut_goal", cap);
            p.array("fin_off", p.l.fin_off, cap + 1);
            p.array("kept", p.l.kept, cap);
        }
        {
            Probe<PoseCutRowScratch> p("pose_cut_row", cap);
            p.array("row_xy", p.l.row_xy, cap);
            p.array("row_id", p.l.row_id, cap);
            p.array("row_h", p.l.row_h, cap);
        }
        for (bool headings : {false, true}) {
            Probe<KeepScratch, bool> p(headings ? "keep_dubins" : "keep", cap, headings);
            p.array("live_vcost", p.l.live_vcost, cap);
            p.array("live_nodes", p.l.live_nodes, cap);
            p.array("live_id", p.l.live_id, cap);
            if (headings) p.array("live_heading", p.l.live_heading, cap);
            else if (p.l.live_heading) std::abort();
        }
        {
            const size_t cap8 = (cap + 7) / 8 * 8;
            Probe<KeepTmpScratch> p("keep_tmp", cap);
            p.array("anc0", p.l.anc[0], cap8);
            p.array("anc1", p.l.anc[1], cap8);
            p.array("ok0", p.l.ok[0], cap8);
            p.array("ok1", p.l.ok[1], cap8);
            p.array("count", p.l.count, 2);
        }
        {
            Probe<SeedTmpScratch> p("seed_tmp", cap);
            p.array("rank", p.l.rank, cap);
            p.array("new_parent", p.l.new_parent, cap);
            p.array("err", p.l.err, 2);
        }
    }
    return 0;
}
