// k_pivot_view.h -- included by k_pivot.hip inside the namespace of each kernel family (no include guard: once per family).
// The descriptor view and the lane-0 predicate of that family (blu_dev.h):
//   pv_single (k_pivot_loop)     DevGPDietT<true>: parameters, capacities and six array bases fetched from the descriptor where
//                                they are used; lane == 0 computed where it is used (uniform_here); every array and line view
//                                indexed by a 32-bit byte offset off its scalar base (Arr32, RecField32, LinkField32, ColdArr32)
//   pv_single_w64 (k_pivot_loop_w64)  DevGPDietT<false>: the same view with pointers indexed in 64 bits, for a launch whose
//                                storage reaches 4 GB in one array (BLU_ADDR_WIDE; the host chooses before every launch)
//   pv_wave, pv_wave2 (a batch)  DevGP: everything held, the plain predicate -- these kernels compile as they did before the
//                                diet: with it the 50k-size leg of a batch was 1.4 % slower
// k_pivot.hip, compiled for every family, writes the predicate LANE_IS0(lane); k_pivot_fast.hip is k_pivot_loop's alone and
// calls lane_is0.
#undef LANE_IS0
#if BLU_CFG_WAVE
#define LANE_IS0(lane) ((lane) == 0)
#else
#if BLU_ADDR_WIDE
typedef DevGPDietT<false> DevGP;
#else
typedef DevGPDietT<true> DevGP;
#endif
// (the link views as this family's functions name them: list_remove1, LinksG)
typedef DevGP::AF::LinkF LinkF;
typedef DevGP::AF::LinkB LinkB;
__device__ __forceinline__ bool lane_is0(int lane) { return lane == uniform_here(0); }
#define LANE_IS0(lane) lane_is0(lane)
#endif
