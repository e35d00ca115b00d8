"""Mirror of the reference's `data.ray_utils`, the on-disk format readers, and the device-resident scene that stands in for its dataset
classes' sample assembly (file decoding and resizing stay with the caller)."""
from .scene import DeviceScene      # noqa: F401
