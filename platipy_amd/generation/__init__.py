"""Drop-in for platipy/imaging/generation: masks (mask.py), synthetic deformation fields (dvf.py), deformable
augmentation (augment.py) and inserted shapes (image.py)."""
from . import augment, dvf, image, mask  # noqa: F401
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
from .image import insert_cylinder, insert_cylinder_image, insert_sphere, insert_sphere_image  # noqa: F401
from .mask import extend_mask, get_bone_mask, get_external_mask  # noqa: F401
