// Head_dim-64 attention with compact queries (dl_attn_fwd_q / dl_attn_bwd_q): the CompactQ
// instantiations of the kernel templates in attention.hip and their entry points, in a translation
// unit (and so a code object) of their own.  attention.hip says why.
#define DL_ATTN_COMPACT_Q_UNIT
#include "attention.hip"
