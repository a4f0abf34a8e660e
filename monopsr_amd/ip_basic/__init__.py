"""IP-Basic depth completion (src/ip_basic of the reference) on the GPU: csrc/depth_fill.hip."""
