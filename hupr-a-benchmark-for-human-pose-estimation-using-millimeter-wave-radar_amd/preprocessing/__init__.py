from .cfar import cfar_alpha_table, cfar_detect  # noqa: F401
from .interference import InterferenceFilter, adc_interference, interference_setting  # noqa: F401
from .points import PointCloudSettings, check_points, radar_geometry, radar_point_cloud  # noqa: F401
from .process_iwr1843 import (RadarObject, dca1000_frames, fft_chain, fft_chain_loader, fft_chain_loader_means,  # noqa: F401
                              loader_normalize)
