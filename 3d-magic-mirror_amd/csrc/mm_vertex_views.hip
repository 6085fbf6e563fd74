// mm_vertex_views.hip -- the vertex stage's kernels for multi-view calls (mm_render_views_*): mm_vertex.hip compiled a second time, its
// kernels and launchers under the names *_views, reading every image's vertices from its sample's row (see the head of mm_vertex.hip).
#define MM_VERTEX_VIEWS 1
#include "mm_vertex.hip"
