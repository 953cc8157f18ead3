"""MI355X-native dense-Farneback-flow -> k-means hot path behind the reference's own entry points
(menmitsu/opticalFlowClustering, k-means-color-clustering/).  See DESIGN.md / INTEGRATION.md."""
__version__ = "0.1.0"

from .flow import (OPTFLOW_FARNEBACK_GAUSSIAN, OPTFLOW_USE_INITIAL_FLOW, calcOpticalFlowFarneback,  # noqa: E402,F401
                   clear_farneback_cache)
from . import photometric  # noqa: E402,F401
from . import repair  # noqa: E402,F401
