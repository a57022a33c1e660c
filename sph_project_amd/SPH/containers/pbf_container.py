from sph_project_amd import _lib as F
from .base_container import BaseContainer, _FieldView


class PBFContainer(BaseContainer):
    """pbf_container.py of the reference: the two fields PBF.py writes besides the base ones.

    `particle_old_positions` holds the positions at the step's sort (save_old_position, PBF.py:145), `particle_pbf_lambdas`
    the lambdas of the last executed refine iteration (compute_lambda, :68).  Both are sized particle_max_num: the reference
    sizes them with particle_num[None], which is still 0 when its __init__ runs.  The neighbour walk of the refine
    iterations (base_container.py:550-560: centre cell and distances from the current positions, cell ranges from the
    step-start sort) runs on the device."""
    METHOD = "pbf"

    def __init__(self, config, GGUI=False, **engine_opts):
        super().__init__(config, GGUI, **engine_opts)
        self.particle_old_positions = _FieldView(self, F.F_PBF_OLD_POSITION)
        self.particle_pbf_lambdas = _FieldView(self, F.F_PBF_LAMBDA)
