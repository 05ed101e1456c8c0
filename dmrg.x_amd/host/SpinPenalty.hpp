/** @file SpinPenalty.hpp
    Total-spin penalty (engine extension): -spin_penalty l0,l1,... / -spin_penalty_warmup l.  With a weight l > 0 a step solves
        H' = H + l S-_tot S+_tot,    S- S+ = S^2 - Sz (Sz + 1),
    which in the sector Sz = M shifts every state of spin S by l [S (S + 1) - M (M + 1)] and leaves S = |M| where it is.  Every block carries
    S+_blk = sum of Sp(i) over its sites next to its H (Block::SpinBase::SpTot: built by KronEye_Explicit, rotated by RotateOperators, never
    pruned); the superblock takes (S- S+)_L and (S- S+)_R into copies of H_L and H_R and the two cross terms as plan terms
    (KronBlocks_t::KronSumConstruct).  The blocks stay those of H, so the weight may change from sweep to sweep. */
#ifndef DMRGX_HOST_SPIN_PENALTY_HPP
#define DMRGX_HOST_SPIN_PENALTY_HPP

#include "Noise.hpp"

namespace dmrgx_host {

/** One weight per sweep, read like -noise and -msweeps: the last value holds for every later sweep; the warm-up has its own (default 0). */
typedef NoiseSchedule SpinPenaltySchedule;

/** Reads -spin_penalty and -spin_penalty_warmup.  Values that are negative, not finite or no numbers are refused with
    PETSC_ERR_ARG_OUTOFRANGE; a non-zero weight on more than one rank with PETSC_ERR_SUP.  All zeros is a run without the option. */
inline PetscErrorCode ReadSpinPenaltyOptions(MPI_Comm comm, PetscMPIInt mpi_size, SpinPenaltySchedule& out)
{
    PetscErrorCode ierr = ReadSweepWeights(comm, "-spin_penalty", "-spin_penalty_warmup", out); CHKERRQ(ierr);
    if (out.Any() && mpi_size > 1)
        SETERRQ1(comm, PETSC_ERR_SUP, "-spin_penalty is not available on more than one rank (got %d): the carried total-spin operator and the penalised block Hamiltonians are not striped.", (int)mpi_size);
    return 0;
}

}  // namespace dmrgx_host
#endif
