from sph_project_amd import _lib as F
from ..containers import IISPHContainer
from .base_solver import BaseSolver


class IISPHSolver(BaseSolver):
    """IISPH.py of the reference (implicit incompressible SPH: relaxed-Jacobi pressure solve, omega 0.2, at most 20
    iterations, stop when the average density error drops below eta = 0.001, :12-14).

    One deviation, in a term all-fluid scenes never reach: for a rigid neighbour, compute_dii (IISPH.py:40-44) divides by
    rho_i^2, the density compute_density wrote for particle i in this step, where the reference reads
    particle_densities_star[p_i] -- a value it computes only afterwards (zero on the first step: division by zero) and
    which its particle sort does not move (another particle's value from then on).  rho_i is what the IISPH paper's d_ii
    uses.  Single GPU only: a sharded container fails in prepare()."""

    def __init__(self, container: IISPHContainer):
        super().__init__(container)
        self._max_iterations = 20
        self._eta = 0.001
        self._omega = 0.2

    # the device solve has these constants built in (sph_common.hpp): read-only here
    @property
    def max_iterations(self):
        return self._max_iterations

    @property
    def eta(self):
        return self._eta

    @property
    def omega(self):
        return self._omega

    def prepare_pressure_solve(self):
        """init_step + compute_dii + compute_aii + compute_density_star (IISPH.py:93, :18-90)."""
        self.engine.run_phase(F.PH_IISPH_PREPARE)

    def refine_iteration(self):
        """One iteration of refine (IISPH.py:185-192): compute_dij_pj, compute_sum_i, update_pressure."""
        self.engine.run_phase(F.PH_IISPH_ITERATION)
