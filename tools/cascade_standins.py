"""Stand-ins for the three imports of the reference's cascade_transforms.py that are absent here (batchgenerators,
skimage, acvl_utils), so that tools/make_golden.py can execute the reference's own class bodies.  Each restates the
package's documented behaviour over numpy / scipy.ndimage; parity with the packages themselves is unpinned.
"""
import sys
import types

import numpy as np
from scipy import ndimage as ndi


class AbstractTransform(object):
    def __call__(self, **data_dict):
        raise NotImplementedError("Abstract, so implement")


def ball(radius, dtype=np.uint8):
    n = int(2 * radius + 1)
    z, y, x = np.meshgrid(np.linspace(-radius, radius, n), np.linspace(-radius, radius, n),
                          np.linspace(-radius, radius, n), indexing='ij')
    return np.array(x * x + y * y + z * z <= radius * radius, dtype=dtype)


def binary_dilation(image, footprint=None):
    return ndi.binary_dilation(image, structure=footprint)


def binary_erosion(image, footprint=None):
    return ndi.binary_erosion(image, structure=footprint, border_value=True)


def binary_closing(image, footprint=None):
    return binary_erosion(binary_dilation(image, footprint), footprint)


def binary_opening(image, footprint=None):
    return binary_dilation(binary_erosion(image, footprint), footprint)


def label_with_component_sizes(binary_image, connectivity=None):
    labeled, n = ndi.label(binary_image, structure=np.ones((3,) * binary_image.ndim))
    counts = np.bincount(labeled.ravel(), minlength=n + 1)
    return labeled, {i: int(counts[i]) for i in range(1, n + 1)}


def install():
    """Put the stand-in modules into sys.modules under the names cascade_transforms.py imports."""
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    module("acvl_utils")
    module("acvl_utils.morphology")
    module("acvl_utils.morphology.morphology_helper", label_with_component_sizes=label_with_component_sizes)
    module("batchgenerators")
    module("batchgenerators.transforms")
    module("batchgenerators.transforms.abstract_transforms", AbstractTransform=AbstractTransform)
    module("skimage")
    module("skimage.morphology", ball=ball)
    module("skimage.morphology.binary", binary_erosion=binary_erosion, binary_dilation=binary_dilation,
           binary_closing=binary_closing, binary_opening=binary_opening)
