// k_pivot_view.h -- included by k_pivot.hip inside the namespace of each kernel family (no include guard: once per family).
// The descriptor view and the lane-0 predicate of that family (blu_dev.h):
//   pv_single (k_pivot_loop)     DevGPDiet: parameters, capacities and six array bases fetched from the descriptor where they
//                                are used; lane == 0 computed where it is used (uniform_here)
//   pv_wave, pv_wave2 (a batch)  DevGP: everything held, the plain predicate -- these kernels compile as they did before the
//                                diet: with it the 50k-size leg of a batch was 1.4 % slower
// k_pivot.hip, compiled for every family, writes the predicate LANE_IS0(lane); k_pivot_fast.hip is k_pivot_loop's alone and
// calls lane_is0.
#undef LANE_IS0
#if BLU_CFG_WAVE
#define LANE_IS0(lane) ((lane) == 0)
#else
typedef DevGPDiet DevGP;
__device__ __forceinline__ bool lane_is0(int lane) { return lane == uniform_here(0); }
#define LANE_IS0(lane) lane_is0(lane)
#endif
