from .device_input import DeviceInputPipeline  # noqa: F401
from .raw import RawImages, raw_collate  # noqa: F401
