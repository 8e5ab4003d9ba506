"""Parameter / statistic keys of the C ABI (include/blu_hip.h `enum blu_param`, `enum blu_stat`).

Parameters are the public fields of the reference's `struct LU` (src/lu/lu.rs:11-66);
statistics are its getters (src/lu/lu.rs:398-684).
"""
# status codes (enum Status, src/lib.rs:38-64; numbers = upstream BASICLU)
OK = 0
REALLOCATE = 1
WARNING_SINGULAR_MATRIX = 2
ERROR_INVALID_CALL = -2
ERROR_ARGUMENT_MISSING = -3
ERROR_INVALID_ARGUMENT = -4
ERROR_MAXIMUM_UPDATES = -5
ERROR_SINGULAR_UPDATE = -6
ERROR_OUT_OF_MEMORY = -9
ERROR_DEVICE = -100

PARAM_DROPTOL = 0
PARAM_ABSTOL = 1
PARAM_RELTOL = 2
PARAM_NZBIAS = 3
PARAM_MAXSEARCH = 4
PARAM_PAD = 5
PARAM_STRETCH = 6
PARAM_COMPRESS_THRES = 7
PARAM_SPARSE_THRES = 8
PARAM_SEARCH_ROWS = 9
PARAM_REALLOC_FACTOR = 10

STAT_M = 0
STAT_NUPDATE = 1
STAT_NFACTORIZE = 2
STAT_L_NZ = 3
STAT_U_NZ = 4
STAT_MIN_PIVOT = 5
STAT_MAX_PIVOT = 6
STAT_CONDEST_L = 7
STAT_CONDEST_U = 8
STAT_NORM_L = 9
STAT_NORM_U = 10
STAT_NORMEST_L_INV = 11
STAT_NORMEST_U_INV = 12
STAT_ONENORM = 13
STAT_INFNORM = 14
STAT_RESIDUAL_TEST = 15
STAT_MATRIX_NZ = 16
STAT_RANK = 17
STAT_BUMP_SIZE = 18
STAT_BUMP_NZ = 19
STAT_NSEARCH_PIVOT = 20
STAT_NEXPAND = 21
STAT_NGARBAGE = 22
STAT_FACTOR_FLOPS = 23
STAT_TIME_FACTORIZE = 24
STAT_TIME_SINGLETONS = 25
STAT_TIME_SEARCH_PIVOT = 26
STAT_TIME_ELIM_PIVOT = 27
STAT_UPDATE_COST_DENOM = 28
STAT_RANKDEF = 29
STAT_L_MEM = 30
STAT_U_MEM = 31
STAT_W_MEM = 32
STAT_L_FLOPS = 33
STAT_U_FLOPS = 34
STAT_NFORREST = 35
STAT_PIVOT_ERROR = 36
STAT_R_NZ = 37
STAT_R_FLOPS = 38
STAT_MAX_ETA = 39
STAT_DEV_TIME_PIVOT_LOOP = 40
STAT_DEV_TIME_TOTAL = 41
STAT_DEV_RELAUNCHES = 42
STAT_NSYMPERM_TOTAL = 48
STAT_NFORREST_TOTAL = 49
STAT_DEV_NUNSYMPERM_TOTAL = 59
STAT_UPDATE_COST = 124
# k_pivot_loop, early set-up of a small pivot split over two waves (k_pivot_fast.hip: small_setup_next + small_setup_help).
# Device-only diagnostics like 121..126, which have no names here: not STAT_*, the names of what the oracle answers as well.
DEVSTAT_SETUP_TWO_WAVES = 127   # set-ups of small pivots completed on two waves (equals statistic 123)
DEVSTAT_SETUP_ABANDONED = 128   # hand-overs between the two waves that ran into the bound of a wait (a defect: 0)
DEVSTAT_ADDR_WIDE = 129         # addressing of the last launch of k_pivot_loop: 0 narrow (32-bit offsets), 1 wide (k_pivot_loop_w64; env BLU_ADDR32_LIMIT)
DEVSTAT_NARROW_LAUNCHES = 130   # launches of k_pivot_loop in the last factorize that were narrow (of STAT_DEV_RELAUNCHES)
DEVSTAT_ADDR_EXTENT = 151       # bytes: the largest extent an int index of k_pivot_loop reaches now (line records, arenas, factors);
                                # narrow while it is below BLU_ADDR32_LIMIT (131..150 are the diagnostic build's)
