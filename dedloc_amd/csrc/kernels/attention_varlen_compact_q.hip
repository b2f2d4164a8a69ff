// Head_dim-64 attention with compact queries over packed keys and values (dl_attn_hd64qv_fwd /
// dl_attn_hd64qv_bwd): the VARLEN + CompactQ instantiations of the kernel templates in attention.hip
// and their entry points, in a translation unit (and so a code object) of their own, so that no
// kernel of attention.hip or attention_compact_q.hip moves.  attention.hip says why.
#define DL_ATTN_VARLEN_COMPACT_Q_UNIT
#include "attention.hip"
