// Stand-alone check of one contract-2 env plug-in header on the host: the header (force-included by the build line,
// plain C++, no HIP) and pgm_envplug.hpp, the transition the plug-in library's pgm_envplug_transition_ex evaluates,
// with the runtime parameters and the step's uniforms behind a pgm_env_ctx.  Built with -ffp-contract=off and the
// address / undefined-behaviour sanitizers by tests/test_envplug2.py.
//
// stdin:  "R rows n", then NP parameters, then rows*R*RW table values, then n items
//         "sd[SD] si[SI] elapsed episode row action w[NW]" (floats as C99 hex; the action is A floats, or the action
//         index of a DISCRETE header)
// stdout: per item "sd[SD] obs[O] obj[K] reward | si[SI] elapsed episode done bad", then one line of NW + 1 stream
//         words "u53(7, 0) ... " for the stream restatement
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../pgmorl_amd/csrc/pgm_envplug.hpp"

using namespace pgm::envplug;

static_assert(C2, "this harness is for CONTRACT = 2 headers");

static double rd() {
    char buf[64];
    if (scanf("%63s", buf) != 1) exit(2);
    return strtod(buf, nullptr);
}
static int ri() {
    int v;
    if (scanf("%d", &v) != 1) exit(2);
    return v;
}

int main() {
    const int R = ri(), rows = ri(), n = ri();
    if (R < 1 || rows < 1 || n < 0) return 2;
    std::vector<double> par(NP), table((size_t)rows * R * Env::RW), w(NW);  // exact sizes: an index past NP / NW shows
    for (double& v : par) v = rd();
    for (double& v : table) v = rd();
    for (int i = 0; i < n; ++i) {
        State s = {};
        for (int j = 0; j < Env::SD; ++j) s.sd[j] = rd();
        for (int j = 0; j < Env::SI; ++j) s.si[j] = ri();
        s.elapsed = ri();
        s.episode = ri();
        const int row = ri();
        if (row < 0 || row >= rows || s.episode < 0) return 2;
        float av[Env::A] = {};
        int ai = 0;
        if (Env::DISCRETE) {
            ai = ri();
            if (ai < 0 || ai >= Env::A) return 2;
        } else {
            for (int j = 0; j < Env::A; ++j) av[j] = (float)rd();
        }
        for (double& v : w) v = rd();
        const pgm_env_ctx ctx{NP ? par.data() : nullptr, NW ? w.data() : nullptr};
        const StepOut o = transition(s, Action{av, ai}, table.data() + (size_t)row * R * Env::RW, R, ctx);
        double obs[Env::O];
        call_observe<Env>(s.sd, s.si, obs, ctx.par);
        for (int j = 0; j < Env::SD; ++j) printf("%a ", s.sd[j]);
        for (int j = 0; j < Env::O; ++j) printf("%a ", obs[j]);
        for (int j = 0; j < Env::K; ++j) printf("%a ", o.obj[j]);
        printf("%a |", o.reward);
        for (int j = 0; j < Env::SI; ++j) printf(" %d", s.si[j]);
        printf(" %d %d %d %d\n", s.elapsed, s.episode, o.done, o.bad);
    }
    for (int j = 0; j <= NW; ++j) printf("%a ", u53(7, (uint64_t)j));
    printf("\n");
    fprintf(stderr, "%d cases\n", n);
    return 0;
}
