// The live stream's device-resident session state, shared by the kernels that read it (stream_window.hip, cfar.hip).
#pragma once

namespace hupr {

// frames = sensor-frames pushed so far (= the number of the next frame), emitted = poses emitted so far (= the number of the next
// centre frame once the stream runs; the flush centres count on from it).
struct StreamState {
    int frames;
    int emitted;
    int pad[2];
};

}  // namespace hupr
