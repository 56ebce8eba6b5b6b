// vba_kernels.h -- hand-written HIP kernels (gfx950, wave64) of the local-BA hot path.
//
// One launch = one phase of one outer iteration for EVERY window of the batch (lock-step); a window whose
// optimize() loop has terminated makes its workgroups exit at the first instruction.  All reductions use a
// fixed order (no floating-point atomics): results are bit-reproducible run to run.
#pragma once
#include "vba_device.h"
#include "vba_batch.h"
#include "vba_lin.h"
#include "vba_schur.h"
#include "vba_factor.h"
#include "vba_trsv.h"
#include "vba_update.h"
