from .optim import FusedAdam, FusedSGD  # noqa: F401

_STREAM = ("PoseStream", "PoseFrame", "StreamSchedule", "stream_window_sources", "StreamError", "LookaheadError",
           "FrameShapeError", "FrameDtypeError", "StreamEndedError", "PoseSmoothing", "DecodeError", "SmoothingError",
           "PoseTracking", "TrackedPoseFrame", "PairedPoseFrame", "TrackingError", "PresenceGate", "PresenceError",
           "InterferenceError", "LaggedPose", "LaggedTrackedPoseFrame", "LaggedPairedPoseFrame",
           "ManeuveringPoseFrame")
_SMOOTH = ("SequenceSmoother", "SmoothedSequence", "TrackHistory", "LagRecord", "ManeuverHistory", "jitter")
_CALIBRATE = ("MeasurementRecord", "TrackingFit", "fit_tracking")


def __getattr__(name):          # lazy: Runner pulls in datasets/models
    if name == "Runner":
        from .run import Runner
        return Runner
    if name in _STREAM:         # the live-stream session (tools/stream.py)
        from . import stream
        return getattr(stream, name)
    if name in _SMOOTH:         # offline smoothing of tracked sequences (tools/smooth.py)
        from . import smooth
        return getattr(smooth, name)
    if name in _CALIBRATE:      # fitting the tracker's noise parameters to a recording (tools/calibrate.py)
        from . import calibrate
        return getattr(calibrate, name)
    raise AttributeError(name)
