"""Drop-in for platipy/imaging/generation: masks (mask.py), synthetic deformation fields (dvf.py) and deformable
augmentation (augment.py)."""
from . import augment, dvf, mask  # noqa: F401
from .augment import (  # noqa: F401
    ContractAugment,
    DeformableAugment,
    ExpandAugment,
    ShiftAugment,
    apply_augmentation,
    generate_random_augmentation,
)
from .dvf import (  # noqa: F401
    generate_field_asymmetric_contract,
    generate_field_asymmetric_extend,
    generate_field_expand,
    generate_field_radial_bend,
    generate_field_shift,
)
from .mask import extend_mask, get_bone_mask  # noqa: F401
