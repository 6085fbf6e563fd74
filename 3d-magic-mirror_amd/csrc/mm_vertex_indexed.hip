// mm_vertex_indexed.hip -- the vertex stage's kernels for indexed calls (mm_render_indexed_*): mm_vertex.hip compiled a third time, its
// kernels and launchers under the names *_indexed, reading every image's vertices from the row the plan's table names (see the head of
// mm_vertex.hip).
#define MM_VERTEX_INDEXED 1
#include "mm_vertex.hip"
