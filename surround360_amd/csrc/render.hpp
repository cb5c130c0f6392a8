// render.hpp — device-resident per-frame pipeline state (renderStereoPanorama, TRSP:716-972).
#pragma once
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "core.hpp"
#include "ctx.hpp"
#include "debug_views.hpp"
#include "png.hpp"
#include "render_kernels.hpp"

namespace s360 {

struct Tables {
  DevBuf bi, bf, t10, t5, fs, gik, bw1, bres;
  DevTables dev;
  int gauss_ksize = 0;
  void build(hipStream_t st, int std_alpha_feather_size);
};

// Warp map of bicubicRemapToSpherical for (camera, dst size, angles): built once, cached in HBM.
void build_spherical_map(s360_ctx* c, float2* map, int dw, int dh, const s360_camera& cam, float l, float r, float t,
                         float b);

// Buffers a frame only needs INSIDE one of its own kernel sequences — produced and consumed between two neighbouring
// launches of the same slot — are shared by all frame slots of a context (the slots of a batch take their per-slot kernels
// one after the other on one stream): the side projections (dead once the overlaps are cropped), the flipped panoramas
// and pole projections (dead once the extended flow inputs exist), the pole warp's intermediates and warped layers (dead
// once composited), the composite's ping-pong buffer, the resized eyes (dead once packed). 1.7 GB per 8K slot that 13 of
// 14 slots no longer hold: 2 x 16 slots fit where 2 x 14 did. With several slots the getters of these intermediates
// (s360_frame_get_u8 "projection", "top_spherical", "bottom_spherical", "pole_warped") show the slot rendered last.
struct SlotScratch {
  DevBuf proj;
  DevBuf panoFlip[2], panoTmp;
  DevBuf topSph, botSph;
  DevBuf warpedExt, poleWarped[4];
  // poleWarped[u] is a whole eye (W x H) of which the frame path writes only the layer's own rows: [polePadFrom[u], polePadTo[u])
  // are the bytes behind them that were zeroed (transparent padding) when the buffer was allocated or its layout last changed
  const void* polePadBuf[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t polePadFrom[4] = {0, 0, 0, 0}, polePadTo[4] = {0, 0, 0, 0};
  const void* poleOwner[4] = {nullptr, nullptr, nullptr, nullptr};  // the slot (FrameState) whose frame poleWarped[u] holds: with the
                                                                    // split phases two slots could interleave (frame_composite checks)
  DevBuf warpPacked, warpTiles;  // this frame's pole warp as packed coordinates + tile boxes (launch_pole_warp_packed)
  DevBuf eyeFinal[2];
  DevBuf pngScratch;  // the device PNG encoder's per-band segments before they are gathered into a slot's file image (png.hip)
  // the sharpen passes' 8-bit low-pass image and checkpoint scratch for ONE group of kSharpenGroup images: the eyes of a
  // batch are sharpened group after group on one stream. The passes keep no float image (render_kernels.hip, k_iir_pass),
  // so a group costs 138 MB of low pass + 9 MB of checkpoints per 8K eye
  static constexpr int kSharpenGroup = 32;
  DevBuf sharpLp[kSharpenGroup], sharpBuf[kSharpenGroup];
};

struct FrameState {
  Tables tab;
  std::shared_ptr<SlotScratch> sc;  // the context's (frame_state())
  int P = 0;                       // number of side cameras / pairs
  int srcW = 0, srcH = 0;
  int topW = 0, topH = 0, poleW = 0, poleH = 0;  // top camera image; bottom camera image (poleW/poleH: also pole removal)
  unsigned long long side_uploaded = 0;          // bit i: side camera i has an image (cleared by nothing: images persist)
  bool have_side = false, have_top = false, have_bottom = false;
  DevBuf staging, sideSrc, topSrc, botSrc;
  DevBuf overlaps[2];  // [cur/prev] temporal double buffer of the flow INPUTS (the motion map needs this frame's and the previous one's)
  // The flows themselves are ONE buffer (round 5): PixFlow reads the previous flow once, at its entry (the downscale into the previous
  // flow's pyramid, PixFlow.h:103-104), and writes the new one once, at its end (the final upscale + blur) — in place on one stream.
  // 1.16 GB less per temporally chained 8K slot (side 0.48 + pole 0.68): two more streams per context.
  DevBuf sideFlows;
  int side_p0 = 0, side_p1 = 0;       // pairs held by overlaps/sideFlows (local partition)
  bool partition_declared = false;    // s360_frame_set_partition was called (set_prev_side then fills that block)
  DevBuf strips;                      // [2][P][camH][stripW]
  DevBuf pano[2];
  DevBuf a8a, a8b, gtmp;
  DevBuf extImgs[2], poleFlows;       // extImgs [cur/prev]; slots: ext 0-3 side units, 4 top fisheye, 5 bottom fisheye; poleFlows: in place

  // Stacked equirect of the last two frames (alternating): a streaming host downloads frame k from one buffer while
  // frame k+1 is composited into the other (s360_frame_download_equirect_of). outDone[i] is recorded behind the
  // kernels that fill outBGR[i].
  DevBuf outBGR[2];
  hipEvent_t outDone[2] = {nullptr, nullptr};
  // device snapshot of the three flow engines' sweep error words, copied on the render stream just in front of
  // outDone[i]; a download's own stream copies it out with the pixels (ctx downErr): s360_frame_download_equirect_of refuses a
  // frame whose sweeps timed out without waiting for the frame that renders behind it (the words are cumulative, so a
  // non-zero value may also come from that next frame's side flows — either way the stream's results are invalid from here on)
  DevBuf outErrDev[2];
  // s360_frame_download_equirect_of releases the context while it waits: downRead[i] is recorded on the download stream behind
  // its copy of outBGR[i] / outErrDev[i], and the finish stage that next writes buffer i waits for it (a feeder two frames ahead of
  // the fetching thread must not overwrite a frame that is still being transferred)
  hipEvent_t downRead[2] = {nullptr, nullptr};
  // s360_set_png_encode: the frame in outBGR[i] also as a PNG file image (band chunks at their final offsets, png.hip) and its
  // band table, written by the finish stage in front of outDone[i]; pngFrame[i] = the frame (frames_done) they belong to
  DevBuf pngFile[2], pngMeta[2];
  PngPlan pngPlan[2];
  long long pngFrame[2] = {-1, -1};
  int out_cur = 0;           // buffer of the most recently ENQUEUED frame
  long long frames_done = 0;  // frames enqueued so far
  long long poleFrame[4] = {-1, -1, -1, -1};  // the frame (value of frames_done) pole unit u's warped layer was computed / received for
  ~FrameState() {
    for (auto& e : outDone) if (e) (void)hipEventDestroy(e);
    for (auto& e : downRead) if (e) (void)hipEventDestroy(e);
  }
  int cur_side = 0, cur_pole = 0, last_side = 0, last_pole = 0;
  bool have_prev_side = false, have_prev_pole = false;
  // previous state handed in in halves (s360_frame_set_prev_images_png / s360_frame_set_prev_flow): what has arrived so far per
  // pair (bits: overlap_l, overlap_r, flow_l_to_r, flow_r_to_l), per pole unit (extended_side, extended_fisheye, flow_pole) and for
  // pole removal (bottom_image, bottom_image2, flow_bottom_secondary); a complete set marks the state as handed in and is cleared
  std::vector<unsigned char> prevSideGot;
  unsigned char prevPoleGot[4] = {0, 0, 0, 0}, prevPrGot = 0;
  int prevPrW = 0, prevPrH = 0;  // size of the pole-removal images handed in as files
  bool keep_intermediates = false;  // copy panoramas before the pole composite (parity tests)
  DevBuf panoDbg[2];
  int extW = 0, poleRowsT = 0, poleRowsB = 0;  // geometry the pole temporal state was produced with (its layout: PrevLayout below)
  // pole removal: secondary bottom source (BGRA), red-mask planes, flow inputs [cur/prev][2][n], flow [cur/prev][n]
  DevBuf botSrc2, prRed[2], prImgs[2], prFlow[2], prTmp, prWarp, prMerged;
  bool have_pr_inputs = false, have_prev_pr = false;
  // the secondary bottom image handed in as a camera (S360_CAMERA_BOTTOM2 / s360_frame_upload_bottom2) and its size
  bool have_bottom2 = false;
  int bot2W = 0, bot2H = 0;
  int last_pr = 0;
  DevBuf cubeOut;  // s360_frame_cubemap's stacked BGR cubemap (the face maps are the context's: ctx.hpp CubeMaps)
  // s360_set_cubemap_output: the stacked cubemap of the frame in outBGR[i] (the finish stage renders it behind the sharpen and in
  // front of outDone[i]; outDone / downRead cover both outputs), its size, the frame (frames_done) it belongs to, and with
  // s360_set_png_encode its file image. Allocated only while the feature is on.
  DevBuf cubeBGR[2];
  int cubeOutW[2] = {0, 0}, cubeOutH[2] = {0, 0};
  long long cubeFrame[2] = {-1, -1};
  DevBuf cubePngFile[2], cubePngMeta[2];
  PngPlan cubePngPlan[2];
  long long cubePngFrame[2] = {-1, -1};
  // s360_set_jpeg_encode: the frame in outBGR[i] / cubeBGR[i] also as the scan of a baseline JPEG file (jpeg.hip), written by the
  // finish stage in front of outDone[i]. k = 0 the equirect, 1 the cubemap. scan: jpeg_frame_scan_cap bytes, NOT the format's worst
  // case; count[i]: two device words, each scan's size in bytes — larger than cap when the scan did not fit and was not stored;
  // countPin[i]: their copy in page-locked memory, valid once outDone[i] has fired (a fetch then knows the size before it
  // enqueues its copy); hdr: the 623 bytes in front of the scan, kept with the frame so that a change of quality or size never
  // mixes tables; frame: the frame (frames_done) all that belongs to. Allocated only while the feature is on.
  struct JpegOut {
    DevBuf scan[2];
    size_t cap[2] = {0, 0};
    std::vector<uint8_t> hdr[2];
    long long frame[2] = {-1, -1};
  } jpeg[2];
  DevBuf jpegCount[2];
  PinBuf jpegCountPin[2];
  // s360_set_debug_images (include/s360_debug_images.h): what the reference's --save_debug_images files of this slot's latest frame
  // are read from. Most of them are buffers the frame leaves behind anyway (projections, pole projections, warped layers, extended
  // side images, pole removal's images: `list` points at them); kept apart are the panoramas before the pole composite (panoDbg,
  // shared with keep_intermediates) and, with sharpening, the eyes before the sharpen overwrites them (eyeKeep); `views` holds what
  // ONE k_debug_views launch behind the frame's last kernel writes through `table`: the cropped feathered side images, the
  // offset-wrapped panoramas, the eyes without alpha. Nothing of this is allocated while the switch has never been on.
  struct DebugImages {
    struct Img { char name[96]; int w, h, ch; const uint8_t* px; };
    std::vector<Img> list;  // in the order of include/s360_debug_images.h
    long long frame = -1;   // the frame (frames_done at its finish stage) the list describes; -1: none
    DevBuf eyeKeep[2], views, table;
    PinBuf tableHost;
  } dbg;
};

// kExtendFrac (TRSP:400-401, 507): the pole stage's images are the panorama extended to this many widths, x % cols
constexpr float kExtendFrac = 1.2f;
inline int extended_width(int cols) { return int(float(cols) * kExtendFrac); }

// Where a slot's temporal state lies — the one description that the stages that write it (frame_render_pairs, the finish stage)
// and the entry points that hand it in or read it back (s360_frame_set_prev_*, s360_frame_get_*) share. Offsets are in pixels.
//   overlaps[cur/prev] / sideFlows: the block [p0, p0 + n) of pairs: L images / LtoR flows of the block first, then R / RtoL
//   extImgs[cur/prev]: six slots of `xs` pixels: the extended side images of pole units 0-3 (0 top_left, 1 top_right,
//                      2 bottom_left, 3 bottom_right), then the top and the bottom extended fisheye image
//   poleFlows: four slots of `xs` pixels, one per unit
struct PrevLayout {
  size_t on;              // one overlap image / side flow
  int p0, n;
  int extW, rowsT, rowsB;
  size_t xs;              // slot stride of extImgs / poleFlows: room for the taller pole
  explicit PrevLayout(const s360_ctx* c, int p0_ = 0, int p1 = 0)  // (no pairs: the pole half alone)
      : on((size_t)c->g.overlap_image_width * c->g.cam_image_height), p0(p0_), n(p1 - p0_), extW(extended_width(c->P.eqr_width)),
        rowsT(c->g.top_rows), rowsB(c->g.bottom_rows), xs((size_t)extW * std::max(rowsT, rowsB)) {}
  size_t left(int j) const { return on * j; }         // pair p0 + j: overlap_l / flow_l_to_r
  size_t right(int j) const { return on * (n + j); }  // ... overlap_r / flow_r_to_l
  int rows(int unit) const { return unit < 2 ? rowsT : rowsB; }
  size_t unit_pixels(int unit) const { return (size_t)extW * rows(unit); }
  size_t side(int unit) const { return xs * unit; }                   // extended side image of a unit; also its flow in poleFlows
  size_t fisheye(int unit) const { return xs * (unit < 2 ? 4 : 5); }  // the fisheye image is shared by the two units of a pole
  size_t overlaps_bytes() const { return 2 * n * on * sizeof(uchar4); }
  size_t side_flows_bytes() const { return 2 * n * on * sizeof(float2); }
  size_t ext_bytes() const { return 6 * xs * sizeof(uchar4); }
  size_t pole_flows_bytes() const { return 4 * xs * sizeof(float2); }
  // the geometry the pole state of F was produced with (what the getters report and the finish stage compares)
  void stamp_pole(FrameState& F) const { F.extW = extW; F.poleRowsT = rowsT; F.poleRowsB = rowsB; }
};

FrameState& frame_state(s360_ctx* c);
void frame_upload_side(s360_ctx* c, int idx, const uint8_t* img, int w, int h, int ch);
void frame_upload_pole(s360_ctx* c, bool top, const uint8_t* bgr, int w, int h);
void frame_upload_raw(s360_ctx* c, struct s360_isp* isp, int which, const void* raw, int bits, int inW, int inH);
void frame_upload_pole_removal(s360_ctx* c, const uint8_t* bottom2, const uint8_t* mask, const uint8_t* mask2, int w, int h);
// include/s360_pole_inputs.h: the secondary bottom camera's pixels; the masks as state of the context (nullptr: cleared)
void frame_upload_bottom2(s360_ctx* c, const uint8_t* bgr, int w, int h);
void set_pole_masks(s360_ctx* c, const uint8_t* mask, const uint8_t* mask2, int w, int h);
// may `camera` be named in an upload call of this context? (side index, S360_CAMERA_TOP / _BOTTOM; S360_CAMERA_BOTTOM2 with pole removal)
bool upload_camera_valid(const s360_ctx* c, int camera, int P);
// the size rules of the two bottom sources before anything is enqueued: (bw, bh) / (b2w, b2h) = the bottom / secondary image of this
// call, 0 = not part of it. Throws S360_ERR_INVALID_ARG.
void check_bottom_sizes(s360_ctx* c, int bw, int bh, int b2w, int b2h);
// cams[i]: side index, S360_CAMERA_TOP, S360_CAMERA_BOTTOM or (pole removal) S360_CAMERA_BOTTOM2; info[i]: files[i] parsed (png_parse_banded_input), 3 channels
void frame_upload_png(s360_ctx* c, const std::vector<int>& cams, const std::vector<const uint8_t*>& files,
                      const std::vector<PngBandedInfo>& info);
// ... and the same from baseline JPEG files (include/s360_input_jpeg.h); info[i]: files[i] parsed (jpeg_in_parse)
void frame_upload_jpeg(s360_ctx* c, const std::vector<int>& cams, const std::vector<const uint8_t*>& files,
                       const std::vector<JpegInInfo>& info);
void frame_render_pairs(s360_ctx* c, int p0, int p1, int use_prev);
void frame_finish(s360_ctx* c, int pole_mask, int use_prev);
// the two halves of frame_finish for a frame whose pole units are spread over GPUs
void frame_pole_units(s360_ctx* c, int pole_mask, int use_prev);
void frame_composite(s360_ctx* c, int pole_mask);
// all slots at once: per-frame kernels slot by slot, the side flows of all slots in one FlowEngine batch, the pole
// flows of all slots in another
void frame_render_batch(s360_ctx* c, int use_prev);
void frame_render_slots(s360_ctx* c, const int* slots, int n, int use_prev);  // ... a subset of them (ascending, distinct)
void set_frame_slots(s360_ctx* c, int n);
// s360_set_debug_images: c->debug_images = on, with what it implies for the context (no pipelining, one slot; streams idle afterwards)
void set_debug_images(s360_ctx* c, bool on);
// The context's frame JPEG encoder (s360_set_jpeg_encode), created on first use and grown to `mcus` MCUs of 16 x 16 pixels; its
// tables are those of the context's quality when this returns. Waits for the device when it has to build or rebuild anything.
JpegEncoder& frame_jpeg_encoder(s360_ctx* c, long long mcus, hipStream_t st);
// stereo cubemap of the last finished frame into F.cubeOut; returns its width/height through ow/oh
void frame_cubemap(s360_ctx* c, int face_w, int face_h, bool video, int* ow, int* oh);
// the context's face maps for (face size, eye size), with their prepared form for `video` (0 / 1) when video >= 0: built on
// first use (host arithmetic, upload, pack kernel, host wait), then shared by every slot and stream
s360_ctx::CubeMaps& cube_maps(s360_ctx* c, int face_w, int face_h, int video);
// ... and their host arithmetic alone: 6 x face_h x face_w x 2 floats for eyes of W x H (what cube_maps uploads; the test tap of
// include/s360_debug_cubemap.h builds its own through it)
std::vector<float> cube_face_maps(int W, int H, int face_w, int face_h);

// RCCL strip gather of the sharded frame (comm.cpp)
void comm_unique_id(void* id128);
const char* comm_library_path();  // the file the RCCL entry points were resolved from (S360_RCCL_LIB overrides the search)
void comm_init_rank(s360_ctx* c, const void* id128, int rank, int nranks);
void comm_init_all(s360_ctx* const* ctxs, int n);
void comm_destroy(s360_ctx* c);
int comm_size(s360_ctx* c);  // ncclCommCount of the context's communicator (0: none)
int comm_rank(s360_ctx* c);  // ncclCommUserRank (-1: none)
void frame_gather_strips(s360_ctx* c, const int* bounds, int root);
void frame_exchange_strips(s360_ctx* c, const int* bounds, const int* need_mask);
void frame_gather_pole_layers(s360_ctx* c, const int* owner, int root);
void comm_loopback(s360_ctx* c, int src_pair, int dst_pair);

// operator-level helpers on device buffers
// erode_size < 0: the context's std_alpha_feather_size and its cached Gaussian taps; otherwise `taps` (device, erode_size ints)
void dev_feather_alpha_to_ext(s360_ctx* c, const uchar4* pano_top_rows, int cols, int rows, uchar4* ext, int extW,
                              int erode_size = -1, const int* taps = nullptr);
std::vector<int> feather_gauss_taps(int erode_size);
// pad_rows: the rows of warped_out below the layer's own are written too (transparent black); the frame path keeps them zeroed itself
void dev_pole_unit_post(s360_ctx* c, const uchar4* extFisheye, const float2* flow, int cols, int rows, int extW,
                        uchar4* warped_out /*cols x eqrH*/, int eqrH, bool pad_rows = true);
// S360_COMPOSITE_FUSED=0: the pole layers are composited one k_flatten launch each, as before k_composite_poles_v4 (A/B runs
// and tests; results do not depend on it). Read once per process.
bool composite_fused_enabled();

// api.hip: does [p, p + bytes) lie in a buffer from s360_host_alloc (page-locked: uploads need no staging copy)?
bool host_is_pinned(const void* p, size_t bytes);

// The context's flow engines (created on first use). which: 0 side / operator-level, 1 pole, 2 pole removal. Without frame
// pipelining the three never compute at the same time (one stream) and share one set of device buffers (flow.hpp FlowBufs);
// with it the finish stage runs on its own stream, and the pole / pole-removal engines get a set of their own.
FlowEngine& flow_engine(s360_ctx* c, int which);
void flow_engines_follow_pipelining(s360_ctx* c);  // after c->pipeline changed (streams idle)

}  // namespace s360
