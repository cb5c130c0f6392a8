// ctx.hpp — the s360_ctx object behind the C ABI: one per device.
#pragma once
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "core.hpp"
#include "flow.hpp"
#include "png.hpp"
#include "jpeg.hpp"
#include "jpeg_decode.hpp"
#include "png_decode.hpp"
#include "rig.hpp"

namespace s360 {
struct FrameState;   // render.hpp
struct SlotScratch;  // render.hpp: buffers shared by the frame slots of a context
}

struct s360_ctx {
  // Every C-ABI entry point that takes a context holds this lock for its whole duration (api_guard.hpp `guard`): a context is
  // safe to call from any number of host threads — the 14 std::threads of TRSP:320-335 may share one — and the calls
  // execute one after the other in lock order. Recursive: batch entry points call the single-pair ones.
  mutable std::recursive_mutex mu;
  int device = 0;
  unsigned long long uid = 0;  // unique per process, never reused (what an ISP object binds to)
  hipStream_t st = nullptr;
  // what s360_stream() hands out: the stream created with the context, never swapped (frame_finish replaces `st` by `st2`
  // for its own duration when frame pipelining is on)
  hipStream_t st_user = nullptr;
  // Frame pipelining (s360_set_frame_pipelining): the pole stage / composite (frame_finish) runs on st2 so that it
  // overlaps the side stage (frame_render_pairs) of the NEXT frame of a video stream. The two stages share three
  // things, each guarded by an event: the strips, the pole source images, and the order side(k) -> finish(k).
  hipStream_t st2 = nullptr;
  bool pipeline = false;
  bool two_outputs = false;  // s360_set_output_double_buffer: finished frames alternate between two output buffers without pipelining
  hipEvent_t evSideDone = nullptr, evStripsFree = nullptr, evPoleSrcFree = nullptr;
  bool haveStripsFree = false, havePoleSrcFree = false;
  // Uploads (s360_frame_upload_*) never touch the render streams: the caller's buffer is copied through a small ring
  // of library-owned pinned chunks and sent on stUp, so a host thread can feed frame k+1 while frame k renders. Three
  // events order the two sides: evUploaded (render waits for the inputs), evSideSrcFree / evPoleSrcFree (the upload's
  // conversion kernels wait until the previous frame's projections have read the source images).
  hipStream_t stUp = nullptr;
  hipStream_t stDown = nullptr;  // s360_frame_download_equirect_of: device -> host copy of a finished frame
  hipEvent_t evDown = nullptr;   // ... and what its host thread sleeps on with the context lock released
  s360::PinBuf downErr;          // ... and that frame's sweep error words (copied on stDown with the pixels)
  bool png_encode = false;       // s360_set_png_encode: every finished frame is also encoded as a PNG on the device
  s360::PinBuf pngMetaHost;      // landing area of a frame's band table (s360_frame_download_png)
  // s360_set_jpeg_encode: every finished frame is also encoded as a baseline JPEG on the device (jpeg.hip). ONE encoder per context,
  // created by the first frame that needs it (render.hip frame_jpeg_encoder) and sized for the larger of the equirect and the
  // cubemap: the encodes of a step are serial on the finish stream anyway. Nothing of it exists while the switch has never been on.
  bool jpeg_encode = false;
  int jpeg_quality = 95;
  s360::JpegEncoder frameJpeg;
  s360::PinBuf jpegDown;  // landing area of a frame's scan size when the fetch could not know it up front (s360_frame_download_jpeg)
  // A batch of PNG files encoded by one launch sequence (png_batch_enqueue): the state images of a frame
  // (s360_frame_encode_state_pngs -> statePng) and the operator form (s360_encode_png_batch -> opPng). Buffers are allocated on
  // first use, grow only, and belong to the context. `gen` counts the encode calls: a fetch that finds another batch after its
  // wait reports S360_ERR_STATE instead of mixing two batches.
  struct PngBatch {
    s360::PngBatchPlan plan;
    s360::DevBuf table, scratch, meta, files;
    s360::PinBuf tabHost;   // the table as it is uploaded
    s360::PinBuf metaHost;  // the band tables of all images, copied behind the gather
    hipEvent_t evEnc = nullptr, evRead = nullptr;  // behind the band tables' copy / behind the latest fetch's copy
    hipEvent_t evAfter = nullptr;                  // frame pipelining: orders the encode behind the finish stream
    bool haveEnc = false, haveRead = false, events = false;
    unsigned long long gen = 0;
  };
  PngBatch statePng, opPng;
  // s360_set_debug_images (include/s360_debug_images.h): frames are rendered one at a time and keep the reference's debug images
  // (render.hpp FrameState::DebugImages); their files are a batch of their own (s360_frame_encode_debug_pngs -> debugPng)
  bool debug_images = false;
  PngBatch debugPng;
  // the PNG decoder (png_decode.hip): its buffers (grow only) and the counters of the last decode call on this context
  s360::PngDecodeBufs pngDec;
  unsigned long long pngDecStats[s360::kPngDecodeStatWords] = {0};
  int pngDecFailImage = -1, pngDecFailReason = 0;  // s360_png_decode_failure: of the last decode call
  // the JPEG decoder (jpeg_decode.hip): its buffers (grow only), the counters and the failure of the last decode call on this context
  s360::JpegDecodeBufs jpegDec;
  s360::JpegDecodeStats jpegDecStats;
  int jpegDecFailImage = -1, jpegDecFailReason = 0;
  hipEvent_t evUpHost = nullptr; // s360_frame_uploads_complete
  static constexpr int kPinChunks = 4;
  static constexpr size_t kPinChunkBytes = (size_t)8 << 20;
  void* pin[kPinChunks] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t pinEv[kPinChunks] = {nullptr, nullptr, nullptr, nullptr};
  bool pinUsed[kPinChunks] = {false, false, false, false};
  int pinNext = 0;
  hipEvent_t evUploaded = nullptr, evSideSrcFree = nullptr;
  bool haveUploaded = false, haveSideSrcFree = false;
  // RCCL communicator of the sharded frame (comm.cpp); opaque here so that only comm.cpp needs rccl.h
  void* comm = nullptr;
  int comm_rank = 0, comm_size = 1;
  // what the two exchanges of the sharded frame have moved since the communicator was made (s360_comm_stats):
  // [0] s360_frame_exchange_strips, [1] s360_frame_gather_pole_layers
  struct CommStats { unsigned long long calls = 0, sent = 0, received = 0; } comm_stats[2];
  s360::Rig rig;
  s360_params P;
  s360_geometry g;
  s360::PoleRamp ramp;
  int top_idx = -1, bottom_idx = -1;
  s360::Profiler prof;
  std::unique_ptr<s360::FlowEngine> flow;       // operator-level calls + side flows
  std::unique_ptr<s360::FlowEngine> flow_pole;  // pole flows (different sizes: keeps both buffer sets resident)
  std::unique_ptr<s360::FlowEngine> flow_pr;    // pole-removal flow between the two bottom cameras
  int sweep_mode = -1;  // -1 default (lockstep), 2 latency, 3 throughput (s360_set_sweep_mode)
  std::string err;
  std::string frame_invalid;  // why the flags describe no renderable frame (s360_create); empty = fine
  // scratch for operator-level calls
  s360::DevBuf op_a, op_b, op_c, op_d, op_e, op_f;
  // Frame slots: slot 0 always exists; s360_set_frame_slots(n) adds more so that n independent frames (n streams of a
  // multi-stream job) are rendered by ONE launch sequence with the flows of all of them in the same batched kernels
  // (s360_frame_render_batch). Uploads / getters / downloads act on the selected slot.
  std::vector<std::shared_ptr<s360::FrameState>> slots;
  std::shared_ptr<s360::SlotScratch> slotScratch;
  int slot = 0;
  // warp maps of bicubicRemapToSpherical per rig camera: depend only on rig + sizes, shared by all slots
  s360::DevBuf sideMaps, topMap, botMap;
  // the same maps as the packed remap reads them (render_kernels.hip): per destination pixel one dword, per 64x16 tile
  // the box of source pixels; they also depend on the SOURCE size, so they are (re)built when that is first seen
  // (a small cache per map, keyed by the source size: slots or streams whose input sizes alternate do not re-pack, and a
  // new size never rebuilds buffers another stream of the context may still read; `ready` orders the users after the pack
  // kernel without a host wait)
  struct PackedMap { s360::DevBuf packed, tiles; int sw = -1, sh = -1; hipEvent_t ready = nullptr; };
  struct PackedCache { std::vector<std::unique_ptr<PackedMap>> e; };
  PackedCache sidePk, topPk, botPk;
  // s360_set_cubemap_output: every finished frame also leaves its stereo cubemap (0 x 0 = off). The face warp maps depend
  // only on the sizes: one entry per (face size, eye size) for all slots — the float maps [6][fh][fw] as the host computes them
  // (also what s360_frame_cubemap reads) and, per format (0 photo, 1 video), their prepared form for k_cubemap_tiles. Entries are
  // built with a host wait and never rebuilt or freed before the context is: a frame in flight may still read the one it was
  // enqueued with.
  int cube_fw = 0, cube_fh = 0, cube_video = 1;
  struct CubeMaps { int fw = 0, fh = 0, W = 0, H = 0, lds_pixels = 0; s360::DevBuf maps, packed[2], tiles[2]; };
  std::vector<std::unique_ptr<CubeMaps>> cubeMaps;
  bool maps_ready = false;
  // s360_set_pole_masks (include/s360_pole_inputs.h): pole removal's three alpha planes of poleMaskW x poleMaskH bytes, constants of
  // the masks, the rig and std_alpha_feather_size, shared by all slots — [0] the bottom camera's flow input, [1] the secondary camera's
  // (already turned by 180 degrees when the rig says so), [2] the merged image
  s360::DevBuf poleAlpha[3];
  int poleMaskW = 0, poleMaskH = 0;
  bool havePoleMasks = false;
  hipEvent_t evMaps = nullptr;  // behind the kernels that built the float maps (the pack kernels may run on another stream)
  void make_current() const { S360_HIP(hipSetDevice(device)); }
};
