// Stand-alone host program over pgm_dummy.hpp (no HIP, no library): the MO-Dummy transition on the input set that
// tests/test_dummy_device.py writes to stdin, one line per case on stdout.  Built with -fsanitize=address,undefined
// (and -ffp-contract=off: the header's pragma is clang's) by the test, which compares the lines with
// pgm_dummy_transition's outputs.
//   stdin   blocks of: "max_steps tlb bound K R count n", count * R * 2 reset positions, then n cases
//           "px py vx vy dist energy step episode env a0 a1" (floating-point values as C99 hex floats)
//   stdout  per case "px py vx vy dist energy obj0 obj1 obj2 reward step episode done bad"
#include <stdio.h>

#include <vector>

#include "pgm_dummy.hpp"

int main() {
    long cases = 0;
    int ms, tlb, K, R, count, n;
    double bound;
    while (scanf("%d %d %la %d %d %d %d", &ms, &tlb, &bound, &K, &R, &count, &n) == 7) {
        if (R < 1 || count < 1 || n < 0 || (K != 2 && K != 3)) return 2;
        std::vector<double> table((size_t)count * R * 2);  // heap memory for the address sanitizer to watch
        for (double& v : table)
            if (scanf("%la", &v) != 1) return 3;
        for (int i = 0; i < n; ++i) {
            pgm::DummyEnv s;
            int env;
            float a0, a1;
            if (scanf("%la %la %la %la %la %la %d %d %d %a %a", &s.pos[0], &s.pos[1], &s.vel[0], &s.vel[1], &s.dist,
                      &s.energy, &s.step, &s.episode, &env, &a0, &a1) != 11)
                return 4;
            if (env < 0 || env >= count || s.episode < 0) return 5;
            const pgm::DummyOut o =
                pgm::dummy_transition(ms, tlb, bound, K, table.data() + (size_t)env * R * 2, R, s, a0, a1);
            double obs[pgm::DUMMY_OBS];
            pgm::dummy_observe(s, obs);
            printf("%a %a %a %a %a %a %a %a %a %a %d %d %d %d\n", obs[0], obs[1], obs[2], obs[3], obs[4], obs[5], o.obj[0],
                   o.obj[1], o.obj[2], o.reward, s.step, s.episode, o.done, o.bad);
            // invariants that hold for every case
            if (o.bad && !o.done) return 6;
            if (o.done && (s.step != 0 || obs[2] != 0.0 || obs[3] != 0.0 || obs[4] != 0.0 || obs[5] != 0.0)) return 7;
            if (!(o.obj[1] > 0.0 && o.obj[1] <= 10.0)) return 8;
            ++cases;
        }
    }
    fprintf(stderr, "%ld cases\n", cases);
    return 0;
}
