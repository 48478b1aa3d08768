// fps_part.hip -- the split select's workspace and launch (fps_part_kernel: S workgroups per cloud
// run the select rounds together, see FpsPartArgs in fps_select.h).
#include "fps_select.h"

namespace dvcp {

// Workspace of the split select, carved from the caller's buffer: slots [B][2][S][slot] u64 |
// flags [B] u32 + the ticket u32 (padded to 8 bytes) | perm [B][N] u32 | err i32.  The slots,
// flags and ticket are set to all ones per launch.
struct FpsPartWs {
  int64_t slot_bytes, flag_bytes, total;
};
static FpsPartWs fps_part_ws(int B, int N, int S) {
  // a part's slot as fps_select_body lays it out (slotsz there): header, per-wave T, candidates
  const int64_t slotsz = kPartHdr + kPartMaxWaves + 5 * (kSelMax / S);
  FpsPartWs w;
  w.slot_bytes = static_cast<int64_t>(B) * 2 * S * slotsz * 8;
  w.flag_bytes = (static_cast<int64_t>(B) * 4 + 4 + 7) / 8 * 8;  // B flags, the ticket
  w.total = w.slot_bytes + w.flag_bytes + static_cast<int64_t>(B) * N * 4 + 8;
  return w;
}
int64_t fps_workspace_bytes(int B, int N) {  // the split path's B x N fp32, or the split select's
  int64_t need = static_cast<int64_t>(B) * N * 4;
  for (int S = 2; S <= 8; S *= 2) {
    const int64_t t = fps_part_ws(B, N, S).total;
    need = t > need ? t : need;
  }
  return need;
}

// 1024 threads; a part holds ceil(N / 64 / S) 64-point groups, up to 8 per lane slot: 16384 points
// at S = 2, 32768 at S = 4, 65536 at S = 8.  Roles by ticket, the kernel's own candidate target
// (tools/fps_lab runs the other workgroup sizes, targets and the blockIdx placement).
int launch_fps_part(PointsView<float> v, int B, int N, int npoint, const int64_t* start, int64_t* out_idx,
                    float* out_xyz, float* ws, int64_t ws_bytes, int32_t* err, int S, hipStream_t st) {
  constexpr int NT = kFpsSel1024;
  static_assert(NT / kWave <= kPartMaxWaves, "slot layout of fps_part_ws");
  const FpsPartWs w = fps_part_ws(B, N, S);
  const int groups = ceil_div(ceil_div(N, kWave), S);  // 64-point groups per part (at most)
  if (w.total > ws_bytes || N > kPartMaxN || groups > 8 * (NT / kWave)) return 1;
  uint64_t* slots = reinterpret_cast<uint64_t*>(ws);
  uint32_t* flags = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ws) + w.slot_bytes);
  uint32_t* permw = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ws) + w.slot_bytes + w.flag_bytes);
  if (!err) err = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ws) + w.total - 8);
  if (hipMemsetAsync(slots, 0xFF, static_cast<size_t>(w.slot_bytes + w.flag_bytes), st) != hipSuccess)
    return launch_status("dvcp_fps(part memset)");
  const FpsPartArgs qa{slots, flags, permw, err, S, B, N, kFpsSpinCap, 0, flags + B};
  return fps_for_ppt<2, 4, 8>(ceil_div(groups, NT / kWave), [&](auto p) {
    hipLaunchKernelGGL((fps_part_kernel<decltype(p)::value, NT>), dim3(B * S), dim3(NT), 0, st, v, N, npoint, start,
                       out_idx, out_xyz, qa, nullptr);
    return launch_status("dvcp_fps(part)");
  });
}

}  // namespace dvcp
