// plx_tune.hip -- the switches behind plx_tune(): the process-wide defaults (the shipped configuration) and the
// name table.  Lattices work under a snapshot of the defaults taken when their build starts (Tune in plx_internal.h).

#include "plx_kernels.h"

namespace plx {

Tune g_tune_defaults;
thread_local const Tune *tl_tune = &g_tune_defaults;

const Tunable *tunables()
{
    static const Tunable t[] = {
        {"sort_points", &Tune::sort_points},
        {"insert_dedupe", &Tune::insert_dedupe},
        {"compact_nbr", &Tune::compact_nbr},
        {"vertex_order", &Tune::vertex_order},
        {"blur_vpt", &Tune::blur_vpt},
        {"blur_small", &Tune::blur_small},
        {"splat_direct", &Tune::splat_direct},
        {"blur_narrow", &Tune::blur_narrow},
        {"blur_multi", &Tune::blur_multi},
        {"splat_group", &Tune::splat_group},
        {"splat_wide", &Tune::splat_wide},
        {"blur_fuse", &Tune::blur_fuse},
        {"blur_fuse_vec", &Tune::blur_fuse_vec},
        {"block_path", &Tune::block_path},
        {"unpermute_gather", &Tune::unpermute_gather},
        {"block_e", &Tune::block_e},
        {"block_dense_combine", &Tune::block_dense_combine},
        {"perm_rows", &Tune::perm_rows},
        {"nbr_bitmap", &Tune::nbr_bitmap},
        {"nbr_sliced", &Tune::nbr_sliced},
        {"reference_growth", &Tune::reference_growth},
        {"assign_evid", &Tune::assign_evid},
        {"nbr_seed", &Tune::nbr_seed},
        {"blur_active", &Tune::blur_active},
        {"contract_v", &Tune::contract_v},
        {"splat_first", &Tune::splat_first},
#ifdef PLX_DIAG
        {"splat_ablate", &Tune::splat_ablate},
        {"blur_ablate", &Tune::blur_ablate},
        {"block_ablate", &Tune::block_ablate},
#endif
        {nullptr, nullptr},
    };
    return t;
}

}  // namespace plx
