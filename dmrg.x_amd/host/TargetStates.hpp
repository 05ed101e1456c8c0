/** @file TargetStates.hpp
    Several target states (engine extension): the options -nstates / -state_weights, and the weights a step uses.  The k lowest states of
    the target sector are found one after another (dmrgx_eigs_lowest_orth) and the blocks are truncated with the state-averaged density
    matrix sum_s w_s rho_s (dmrgx_kron_states_expand); the solves stay in DMRGBlockContainer::SingleDMRGStep, the truncation in
    GetTruncation. */
#ifndef DMRGX_HOST_TARGET_STATES_HPP
#define DMRGX_HOST_TARGET_STATES_HPP

#include <cmath>
#include <string>
#include <vector>
#include "petsc_compat.hpp"

namespace dmrgx_host {

constexpr PetscInt max_target_states = 8;

/** -nstates k: 1 <= k <= 8, default 1.  -state_weights w0,...: exactly k numbers, non-negative and finite, not all zero; default: equal
    weights.  `weights` holds them normalised to sum 1. */
struct TargetStates {
    PetscInt k = 1;
    std::vector<double> weights{1.0};

    /** The weights of a step whose sector holds nstates_of_sector states: those of the first k_step = min(k, nstates_of_sector) states,
        renormalised to sum 1 -- equal weights should the states that fit carry none. */
    std::vector<double> StepWeights(PetscInt nstates_of_sector) const
    {
        const PetscInt ks = std::max<PetscInt>(1, std::min<PetscInt>(k, nstates_of_sector));
        std::vector<double> w(weights.begin(), weights.begin() + ks);
        double sum = 0.0;
        for (double x : w) sum += x;
        for (double& x : w) x = sum > 0.0 ? x / sum : 1.0 / (double)ks;
        return w;
    }
    /** "[w0, w1, ...]" for the JSON records */
    static std::string Json(const std::vector<double>& w)
    {
        std::string s = "[";
        char buf[40];
        for (size_t i = 0; i < w.size(); ++i) { snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", w[i]); s += buf; }
        return s + "]";
    }
};

/** Reads -nstates and -state_weights from the options database.  A value out of range, a count of weights other than k, a weight that is
    negative, not finite or no number, and weights that are all zero are refused with PETSC_ERR_ARG_OUTOFRANGE. */
inline PetscErrorCode ReadTargetStatesOptions(MPI_Comm comm, TargetStates& out)
{
    PetscErrorCode ierr;
    out = TargetStates();
    PetscBool set = PETSC_FALSE;
    PetscInt k = 1;
    ierr = PetscOptionsGetInt(NULL, NULL, "-nstates", &k, &set); CHKERRQ(ierr);
    if (set && (k < 1 || k > max_target_states)) SETERRQ2(comm, PETSC_ERR_ARG_OUTOFRANGE, "-nstates takes a number of states from 1 to %lld. Got %lld.", LLD(max_target_states), LLD(k));
    out.k = set ? k : 1;
    out.weights.assign((size_t)out.k, 1.0);
    char raw[4096] = "";
    ierr = PetscOptionsGetString(NULL, NULL, "-state_weights", raw, sizeof raw, &set); CHKERRQ(ierr);
    if (set) {
        out.weights.clear();
        const std::string s(raw);
        size_t pos = 0;
        while (pos <= s.size()) {
            const size_t c = s.find(',', pos);
            const std::string tok = s.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
            char* end = nullptr;
            const double w = strtod(tok.c_str(), &end);
            if (tok.empty() || end == tok.c_str() || *end != 0 || !std::isfinite(w) || w < 0.0)
                SETERRQ1(comm, PETSC_ERR_ARG_OUTOFRANGE, "-state_weights takes non-negative numbers separated by commas, one per state. Got \"%s\".", raw);
            out.weights.push_back(w);
            if (c == std::string::npos) break;
            pos = c + 1;
        }
        if ((PetscInt)out.weights.size() != out.k)
            SETERRQ3(comm, PETSC_ERR_ARG_OUTOFRANGE, "-state_weights takes exactly one weight per state: -nstates is %lld, got %lld weights in \"%s\".", LLD(out.k), LLD((PetscInt)out.weights.size()), raw);
    }
    double sum = 0.0;
    for (double w : out.weights) sum += w;
    if (!(sum > 0.0) || !std::isfinite(sum)) SETERRQ1(comm, PETSC_ERR_ARG_OUTOFRANGE, "-state_weights must not all be zero. Got \"%s\".", raw);
    for (double& w : out.weights) w /= sum;
    return 0;
}

}  // namespace dmrgx_host
#endif
