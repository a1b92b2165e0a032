"""Drop-in for platipy/imaging/generation/augment.py: deformable augmentation of an image and its structures.

Each DeformableAugment produces a (transform, dvf) pair from one of the generators in generation/dvf.py;
apply_augmentation composes them and warps the image and every mask through the composite in ONE gather
(registration.apply_transform_to_set -> pp_resample_set) where the reference makes 1 + M apply_transform calls
(augment.py:65-78).
"""
from abc import ABC, abstractmethod
from collections.abc import Iterable
import random

from ..image import Image
from ..registration.utils import apply_transform_to_set
from ..transform import CompositeTransform, sitkLinear
from .dvf import generate_field_expand, generate_field_shift
from .mask import get_bone_mask


def apply_augmentation(image, augmentation, masks=[]):
    """Apply one DeformableAugment, or an iterable of them, to `image` and `masks` (reference augment.py:33-83).

    Returns (image_deformed, masks_deformed, dvf), or (image_deformed, dvf) when no masks are given; dvf is the SUM of the
    members' fields (:57-60) while the image goes through their COMPOSITION (:62), as the reference has it."""
    if not isinstance(image, Image):
        raise AttributeError("image should be a platipy_amd.Image")

    if isinstance(augmentation, DeformableAugment):
        augmentation = [augmentation]

    if not isinstance(augmentation, Iterable):
        raise AttributeError("augmentation must be a DeformableAugment or an iterable (such as list) of DeformableAugment's")

    transforms = []
    dvf = None
    for aug in augmentation:
        if not isinstance(aug, DeformableAugment):
            raise AttributeError("Each augmentation must be of type DeformableAugment")
        tfm, field = aug.augment()
        transforms.append(tfm)
        # (a new Image: the reference's `dvf += field` adds into the first member's field, which its transform copied; here
        # the transform holds the field itself and must keep its own values)
        dvf = field if dvf is None else dvf + field

    transform = CompositeTransform(transforms)
    del transforms

    image_deformed, masks_deformed = apply_transform_to_set(image, list(masks), transform=transform,
                                                            default_value=int(image.tensor.min()), interpolator=sitkLinear)
    if masks:
        return image_deformed, masks_deformed, dvf
    return image_deformed, dvf


def generate_random_augmentation(ct_image, masks):
    """One random augmentation per mask (reference augment.py:86-141).  Python's `random` is used exactly as the reference
    uses it -- one shuffle of `masks` in place, then per mask a choice and its randint draws in the same order -- so
    random.seed reproduces a draw."""
    random.shuffle(masks)
    # (class, its arguments in the order they are drawn): a list = one randint per axis, a tuple = one randint, True = the bone mask
    three_axes = [(0, 10), (0, 10), (0, 10)]
    augmentation_types = [
        (ShiftAugment, {"vector_shift": [(-10, 10), (10, 10), (-10, 10)], "gaussian_smooth": (3, 5)}),
        (ContractAugment, {"vector_contract": three_axes, "gaussian_smooth": (3, 5), "bone_mask": True}),
        (ExpandAugment, {"vector_expand": three_axes, "gaussian_smooth": (3, 5), "bone_mask": True}),
    ]
    augmentation = []
    for mask in masks:
        aug_class, ranges = random.choice(augmentation_types)
        aug_args = {}
        for arg, value in ranges.items():
            if isinstance(value, list):
                value = [random.randint(lo, hi) for lo, hi in value]
            elif isinstance(value, tuple):
                value = random.randint(value[0], value[1])
            elif arg == "bone_mask" and value:
                value = get_bone_mask(ct_image)
            aug_args[arg] = value
        augmentation.append(aug_class(mask, **aug_args))
    return augmentation


class DeformableAugment(ABC):
    @abstractmethod
    def augment(self):
        """-> (transform, dvf)"""


class ShiftAugment(DeformableAugment):
    def __init__(self, mask, vector_shift=(10, 10, 10), gaussian_smooth=5):
        self.mask = mask
        self.vector_shift = vector_shift
        self.gaussian_smooth = gaussian_smooth

    def augment(self):
        _, transform, dvf = generate_field_shift(self.mask, self.vector_shift, self.gaussian_smooth)
        return transform, dvf


class ExpandAugment(DeformableAugment):
    def __init__(self, mask, vector_expand=(10, 10, 10), gaussian_smooth=5, bone_mask=False):
        self.mask = mask
        self.vector_expand = vector_expand
        self.gaussian_smooth = gaussian_smooth
        self.bone_mask = bone_mask

    def augment(self):
        _, transform, dvf = generate_field_expand(self.mask, bone_mask=self.bone_mask, expand=self.vector_expand,
                                                  gaussian_smooth=self.gaussian_smooth)
        return transform, dvf


class ContractAugment(DeformableAugment):
    def __init__(self, mask, vector_contract=(10, 10, 10), gaussian_smooth=5, bone_mask=False):
        self.mask = mask
        # quirk (augment.py:193): the z, y, x vector is divided by the x, y, z spacing and truncated -- and
        # generate_field_expand divides by the spacing once more
        self.contract = [int(-x / s) for x, s in zip(vector_contract, mask.GetSpacing())]
        self.gaussian_smooth = gaussian_smooth
        self.bone_mask = bone_mask

    def augment(self):
        _, transform, dvf = generate_field_expand(self.mask, bone_mask=self.bone_mask, expand=self.contract,
                                                  gaussian_smooth=self.gaussian_smooth)
        return transform, dvf
