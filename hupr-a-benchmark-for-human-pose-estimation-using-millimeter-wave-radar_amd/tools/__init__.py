from .optim import FusedAdam, FusedSGD  # noqa: F401

_STREAM = ("PoseStream", "PoseFrame", "StreamSchedule", "stream_window_sources", "StreamError", "LookaheadError",
           "FrameShapeError", "FrameDtypeError", "StreamEndedError", "PoseSmoothing", "DecodeError", "SmoothingError",
           "PoseTracking", "TrackedPoseFrame", "TrackingError")


def __getattr__(name):          # lazy: Runner pulls in datasets/models
    if name == "Runner":
        from .run import Runner
        return Runner
    if name in _STREAM:         # the live-stream session (tools/stream.py)
        from . import stream
        return getattr(stream, name)
    raise AttributeError(name)
