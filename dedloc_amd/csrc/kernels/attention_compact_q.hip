// Head_dim-64 attention with compact queries (dl_attn_hd64q_fwd / dl_attn_hd64q_bwd): the CompactQ
// instantiations of the kernel templates in attention.hip and their entry points, in a translation
// unit (and so a code object) of their own.  attention.hip says why.
#define DL_ATTN_COMPACT_Q_UNIT
#include "attention.hip"
