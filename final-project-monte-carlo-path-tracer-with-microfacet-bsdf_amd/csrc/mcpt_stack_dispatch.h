// The dispatch of a traversal kernel template <int STK, bool RETRY, bool SMALL> over the stack flavours (Walk, mcpt_traverse.h), shared by
// the translation units that launch such kernels: mcpt_kernels.hip (the render loop's) and mcpt_rayquery.hip (the occlusion query's).
// Include after mcpt_traverse.h.
#pragma once

#include "mcpt_traverse.h"

namespace mcpt {

// Stack flavour by tree height (see Walk in mcpt_traverse.h): <= 17 levels: 16 LDS entries; <= 20: kStkB; <= kPlainMaxHeight (24): 24; deeper: the retry
// flavour (16 LDS entries, retrace list).  (-DMCPT_LDS_ONLY_STACKS: 24 / 32 / 48-entry LDS stacks for deep trees instead, for A/B measurements;
// -DMCPT_FORCE_RETRY, the checking build: the retry flavour for every tree with -DMCPT_STK_RETRY=4 LDS entries, so that most rays are
// traced again.)  RETRACE: the launch of the retrace kernel, issued right behind a retry-flavour kernel on the same stream.
// The macro reads `S`, the DevScene of the launch, for the small-scene flavour.
constexpr uint32_t kRetraceGrid = 256;
#ifdef MCPT_LDS_ONLY_STACKS
#define MCPT_STACK_DISPATCH(height, KERNEL, RETRACE, ...)                                          \
    do {                                                                                           \
        if ((height) <= 17) hipLaunchKernelGGL((KERNEL<16, false, false>), __VA_ARGS__);           \
        else if ((height) <= 20) hipLaunchKernelGGL((KERNEL<kStkB, false, false>), __VA_ARGS__);   \
        else if ((height) <= 24) hipLaunchKernelGGL((KERNEL<24, false, false>), __VA_ARGS__);      \
        else if ((height) <= 32) hipLaunchKernelGGL((KERNEL<32, false, false>), __VA_ARGS__);      \
        else hipLaunchKernelGGL((KERNEL<kMaxBvhHeight, false, false>), __VA_ARGS__);               \
    } while (0)
#elif defined(MCPT_FORCE_RETRY)
#define MCPT_STACK_DISPATCH(height, KERNEL, RETRACE, ...)                                          \
    do {                                                                                           \
        hipLaunchKernelGGL((KERNEL<kStkRetry, true, false>), __VA_ARGS__);                         \
        RETRACE;                                                                                   \
    } while (0)
#else
#define MCPT_STACK_DISPATCH(height, KERNEL, RETRACE, ...)                                          \
    do {                                                                                           \
        if (S.small) hipLaunchKernelGGL((KERNEL<kSmallStk, false, true>), __VA_ARGS__); /* scene in LDS */ \
        else if ((height) <= 17) hipLaunchKernelGGL((KERNEL<16, false, false>), __VA_ARGS__);      \
        else if ((height) <= 20) hipLaunchKernelGGL((KERNEL<kStkB, false, false>), __VA_ARGS__);   \
        else if ((height) <= kPlainMaxHeight) hipLaunchKernelGGL((KERNEL<24, false, false>), __VA_ARGS__); \
        else {                                                                                     \
            hipLaunchKernelGGL((KERNEL<kStkRetry, true, false>), __VA_ARGS__);                     \
            RETRACE;                                                                               \
        }                                                                                          \
    } while (0)
#endif

}  // namespace mcpt
