// Stand-alone host program over pgm_dst.hpp (no HIP, no library): the Deep Sea Treasure transition on the exhaustive
// input set of tests/test_dst_device.py -- every open cell x action 0..3 x step in {0, 1, max_steps - 2,
// max_steps - 1} x max_steps in {50, 12} x time_limit_is_bad in {0, 1} -- one line per case on stdout.  Built with
// -fsanitize=address,undefined by the test, which compares the lines with pgm_dst_transition's outputs.
#include <stdio.h>

#include <vector>

#include "pgm_dst.hpp"

int main() {
    long cases = 0;
    std::vector<pgm::DstStep> keep;  // heap traffic for the address sanitizer to watch
    for (int ms : {50, 12})
        for (int tlb = 0; tlb < 2; ++tlb)
            for (int r = 0; r < pgm::DST_SIZE; ++r)
                for (int c = 0; c < pgm::DST_SIZE; ++c) {
                    if (!pgm::dst_open(r, c)) continue;
                    for (int a = 0; a < 4; ++a)
                        for (int st : {0, 1, ms - 2, ms - 1}) {
                            const pgm::DstStep o = pgm::dst_transition(ms, tlb, r, c, st, a);
                            keep.push_back(o);
                            printf("%d %d %d %d %d %d | %d %d %d %a %a %a %a %a %a %d %d\n", ms, tlb, r, c, a, st, o.row,
                                   o.col, o.step, o.obs[0], o.obs[1], o.obs[2], o.obj[0], o.obj[1], o.reward, o.done,
                                   o.bad);
                            ++cases;
                        }
                }
    // invariants that hold for every case
    for (const pgm::DstStep& o : keep) {
        if (o.row < 0 || o.row >= pgm::DST_SIZE || o.col < 0 || o.col >= pgm::DST_SIZE || !pgm::dst_open(o.row, o.col)) return 2;
        if (o.done && (o.row || o.col || o.step)) return 3;
        if (o.bad && !o.done) return 4;
        if (o.reward != o.obj[0]) return 5;
    }
    fprintf(stderr, "%ld cases\n", cases);
    return 0;
}
