from sph_project_amd import _lib as F
from .base_container import BaseContainer, _FieldView

# scene keys of the consistent variant (Configuration.pbfVariant: "consistent") -> field of sph_set_pbf_variant's struct, default
PBF_KEYS = {"pbfMaxError": ("max_error", 0.001), "pbfMinIterations": ("min_iterations", 1), "pbfMaxIterations": ("max_iterations", 50),
            "pbfEpsilon": ("epsilon", 1e-6)}


def pbf_variant_of(config):
    """("reference" | "consistent", {setter field: value}) of a scene; ValueError for any other pbfVariant.  Key absent: reference."""
    variant = config.get_cfg("pbfVariant")
    if variant is None:
        variant = "reference"
    if variant not in F.PBF_VARIANTS:
        raise ValueError(f"Configuration.pbfVariant must be \"reference\" or \"consistent\", got {variant!r}")
    opts = {}
    for key, (field, default) in PBF_KEYS.items():
        v = config.get_cfg(key)
        opts[field] = default if v is None else v
    return variant, opts


class PBFContainer(BaseContainer):
    """pbf_container.py of the reference: the two fields PBF.py writes besides the base ones.

    `particle_old_positions` holds the positions at the step's sort (save_old_position, PBF.py:145), `particle_pbf_lambdas`
    the lambdas of the last executed refine iteration (compute_lambda, :68).  Both are sized particle_max_num: the reference
    sizes them with particle_num[None], which is still 0 when its __init__ runs.  The neighbour walk of the refine
    iterations (base_container.py:550-560: centre cell and distances from the current positions, cell ranges from the
    step-start sort) runs on the device.

    Configuration.pbfVariant "consistent" selects the variant of DESIGN.md 27 (pbfMaxError, pbfMinIterations, pbfMaxIterations,
    pbfEpsilon tune its solve); absent or "reference": PBF.py as written.  Under the consistent variant `particle_positions` holds
    the old positions for the whole step, `particle_predicted_positions` the x* of the solve, and `particle_old_positions` is
    refused by the library."""
    METHOD = "pbf"

    def __init__(self, config, GGUI=False, **engine_opts):
        self.pbf_variant, self.pbf_options = pbf_variant_of(config)   # (a bad key raises before a device is opened)
        super().__init__(config, GGUI, **engine_opts)
        if self.pbf_variant != "reference":
            self.engine.set_pbf_variant(self.pbf_variant, **self.pbf_options)
            self.particle_predicted_positions = _FieldView(self, F.F_PREDICTED_POS)
        self.particle_old_positions = _FieldView(self, F.F_PBF_OLD_POSITION)
        self.particle_pbf_lambdas = _FieldView(self, F.F_PBF_LAMBDA)
