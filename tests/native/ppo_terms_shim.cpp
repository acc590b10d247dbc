// extern "C" view of the shared PPO loss terms (pgmorl_amd/csrc/pgm_ppo_terms.hpp) for tests/test_ppo_terms.py:
// built by the host compiler alone, no HIP.
#include "pgm_ppo_terms.hpp"

extern "C" {

void pgm_test_value_loss_term(int n, const float* V, const float* Vold, const float* R, float clip, int clipped,
                              float* grad, float* loss) {
    for (int i = 0; i < n; ++i) {
        const pgm::LossTerm t = pgm::value_loss_term(V[i], Vold[i], R[i], clip, clipped != 0);
        grad[i] = t.grad;
        loss[i] = t.loss;
    }
}

void pgm_test_surrogate_term(int n, const float* ratio, const float* adv, float clip, float* grad, float* loss) {
    for (int i = 0; i < n; ++i) {
        const pgm::LossTerm t = pgm::surrogate_term(ratio[i], adv[i], clip);
        grad[i] = t.grad;
        loss[i] = t.loss;
    }
}

}  // extern "C"
