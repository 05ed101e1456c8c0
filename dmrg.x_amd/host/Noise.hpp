/** @file Noise.hpp
    Density-matrix noise (engine extension; White, PRB 72, 180403): the schedule of -noise / -noise_warmup and the operator list that
    dmrgx_kron_noise_expand takes.  The truncation itself stays in DMRGBlockContainer::GetTruncation. */
#ifndef DMRGX_HOST_NOISE_HPP
#define DMRGX_HOST_NOISE_HPP

#include <cmath>
#include <string>
#include <vector>
#include "petsc_compat.hpp"
#include "dmrgx.h"

namespace dmrgx_host {

/** -noise a0,a1,...: one non-negative weight per sweep, read like -msweeps; the last value holds for every later sweep.
    -noise_warmup a: the weight during the warm-up (default 0).  Without the options every weight is 0. */
struct NoiseSchedule {
    std::vector<double> sweeps;
    double warmup = 0.0;

    bool Any() const { if (warmup > 0.0) return true; for (double a : sweeps) if (a > 0.0) return true; return false; }
    /** the weight of a step: in_warmup, or sweep number sweep_idx (0-based) */
    double At(bool in_warmup, PetscInt sweep_idx) const
    {
        if (in_warmup) return warmup;
        if (sweeps.empty()) return 0.0;
        return sweeps[(size_t)std::min<PetscInt>(std::max<PetscInt>(sweep_idx, 0), (PetscInt)sweeps.size() - 1)];
    }
    /** "[a0, a1, ...]" for DMRGRun.json */
    std::string Json() const
    {
        std::string s = "[";
        char buf[40];
        for (size_t i = 0; i < sweeps.size(); ++i) { snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", sweeps[i]); s += buf; }
        return s + "]";
    }
};

/** Reads a schedule of weights from the options database: `name` a0,a1,... and `name_warmup` a.  A value that is negative or not finite,
    or a token that is no number, is refused with PETSC_ERR_ARG_OUTOFRANGE. */
inline PetscErrorCode ReadSweepWeights(MPI_Comm comm, const char* name, const char* name_warmup, NoiseSchedule& out)
{
    PetscErrorCode ierr;
    out = NoiseSchedule();
    PetscBool set = PETSC_FALSE;
    char raw[4096] = "";
    ierr = PetscOptionsGetString(NULL, NULL, name, raw, sizeof raw, &set); CHKERRQ(ierr);
    if (set) {
        const std::string s(raw);
        size_t pos = 0;
        while (pos <= s.size()) {
            const size_t c = s.find(',', pos);
            const std::string tok = s.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
            char* end = nullptr;
            const double a = strtod(tok.c_str(), &end);
            if (tok.empty() || end == tok.c_str() || *end != 0 || !std::isfinite(a) || a < 0.0)
                SETERRQ2(comm, PETSC_ERR_ARG_OUTOFRANGE, "%s takes non-negative numbers separated by commas, one per sweep. Got \"%s\".", name, raw);
            out.sweeps.push_back(a);
            if (c == std::string::npos) break;
            pos = c + 1;
        }
    }
    PetscReal w = 0.0;
    ierr = PetscOptionsGetReal(NULL, NULL, name_warmup, &w, &set); CHKERRQ(ierr);
    if (set && (!std::isfinite(w) || w < 0.0)) SETERRQ2(comm, PETSC_ERR_ARG_OUTOFRANGE, "%s takes a non-negative number. Got %g.", name_warmup, (double)w);
    out.warmup = set ? (double)w : 0.0;
    return 0;
}

/** Reads -noise and -noise_warmup from the options database (ReadSweepWeights). */
inline PetscErrorCode ReadNoiseOptions(MPI_Comm comm, NoiseSchedule& out) { return ReadSweepWeights(comm, "-noise", "-noise_warmup", out); }

/** Two descriptors of the same operator: the same cells (compared field by field: the plan lists Sp(i) and Sm(i) as two views of one
    set of device blocks) read the same way. */
inline bool SameOperator(const dmrgx_secop& x, const dmrgx_secop& y)
{
    if (x.shift != y.shift || (x.transposed != 0) != (y.transposed != 0) || x.ncells != y.ncells) return false;
    for (int32_t i = 0; i < x.ncells; ++i) {
        const dmrgx_cell &c = x.cells[i], &d = y.cells[i];
        if (c.row_sector != d.row_sector || c.r0 != d.r0 || c.c0 != d.c0 || c.nr != d.nr || c.nc != d.nc || c.kind != d.kind) return false;
        if (c.kind == DMRGX_CELL_DENSE ? (c.data != d.data || c.ld != d.ld) : (c.scale != d.scale)) return false;
    }
    return true;
}

/** The operators of one side of a step's plan as dmrgx_kron_noise_expand takes them: every distinct one as it is, and for every operator
    with a non-zero shift its transpose (Sm beside Sp: the same cells read the other way) unless the list has it already -- a Heisenberg
    term names both Sp(i) and Sm(i), which are each other's transposes --, each with coefficient sqrt(a). */
inline void NoiseOperators(const std::vector<dmrgx_secop>& plan_ops, double a, std::vector<dmrgx_secop>& ops, std::vector<double>& coef)
{
    ops.clear();
    auto add = [&](const dmrgx_secop& o) { for (const dmrgx_secop& e : ops) if (SameOperator(e, o)) return; ops.push_back(o); };
    for (const dmrgx_secop& o : plan_ops) add(o);
    for (const dmrgx_secop& o : plan_ops)
        if (o.shift != 0) { dmrgx_secop t = o; t.shift = -o.shift; t.transposed = o.transposed ? 0 : 1; add(t); }
    coef.assign(ops.size(), std::sqrt(a));
}

}  // namespace dmrgx_host
#endif
