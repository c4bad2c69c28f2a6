"""Every kernel instance in the library's gfx950 code object.  A product call selects each of them, and the rows of
tests/test_gpu_buffer_contract.py reach each of them (a kernel trace of that file lists them all -- see the module docstring there for
the command).

tests/test_kernel_forms_host.py checks that this set is exactly the instances of the built library, so a new form (a new template
instance) must be listed here -- and given a row -- before the suite passes, and a launch rule cannot keep an instance alive that no call
selects.  Names are demangled, without the argument list and without blanks.
"""

PRODUCT = {
    # misc
    "moka_adamw_begin_kernel", "moka_adamw_kernel", "moka_dropout_mask_kernel", "moka_sum_runs_kernel",
    # interaction, shadows
    "moka_cross_bwd_kernel<16>", "moka_cross_bwd_kernel<32>", "moka_cross_bwd_kernel<64>",
    "moka_cross_bwd_keys_kernel<16>", "moka_cross_bwd_keys_kernel<32>", "moka_cross_bwd_keys_kernel<64>",
    "moka_cross_fwd_kernel<16,4,4>", "moka_cross_fwd_kernel<32,4,4>", "moka_cross_fwd_kernel<64,2,4>",
    "moka_shadows_kernel<16>", "moka_shadows_kernel<32>", "moka_shadows_kernel<64>",
    "moka_shadows_batch_kernel<16>", "moka_shadows_batch_kernel<32>", "moka_shadows_batch_kernel<64>",
    # dx / up-projection
    "moka_dxgt_kernel<32,2>", "moka_dxgt_kernel<32,3>", "moka_dxgt_kernel<64,2>", "moka_dxgt_kernel<64,3>", "moka_dxt_kernel<64>",
    "moka_expand_kernel<16,2,false,2,false>", "moka_expand_kernel<16,2,false,3,false>",
    "moka_expand_kernel<16,4,false,1,false>", "moka_expand_kernel<16,4,true,1,false>",
    "moka_expand_kernel<32,4,false,1,true>", "moka_expand_kernel<32,4,true,1,false>",
    "moka_yt_kernel<16>", "moka_yt_kernel<32>", "moka_yt_kernel<64>",
    "moka_yx_kernel<16>", "moka_yx_kernel<32>", "moka_yx_kernel<64>",
    # fp32 storage
    "moka_f32_expand_kernel<false>", "moka_f32_expand_kernel<true>", "moka_f32_reduce_kernel<false>", "moka_f32_reduce_kernel<true>",
    "moka_f32_wgrad_kernel<false>", "moka_f32_wgrad_kernel<true>",
    # up-projection backward
    "moka_gs_kernel<16,false,false>", "moka_gs_kernel<16,true,false>", "moka_gs_kernel<16,true,true>",
    "moka_gs_kernel<32,false,false>", "moka_gs_kernel<32,true,false>", "moka_gs_kernel<32,true,true>",
    "moka_gy_kernel<false,4,false>",
    "moka_gy_kernel<true,8,false>", "moka_gy_kernel<true,8,true>",
    "moka_gy_kernel<true,16,false>", "moka_gy_kernel<true,16,true>",
    # weight gradients
    "moka_wgrad_kernel<16,4,false,1,false>", "moka_wgrad_kernel<16,4,false,1,true>",
    "moka_wgrad_kernel<16,4,false,2,false>", "moka_wgrad_kernel<16,4,false,2,true>",
    "moka_wgrad_kernel<16,4,false,3,false>", "moka_wgrad_kernel<16,4,false,3,true>",
    "moka_wgrad_kernel<16,8,false,1,false>", "moka_wgrad_kernel<16,8,false,1,true>",
    "moka_wgrad_kernel<16,8,true,1,false>", "moka_wgrad_kernel<16,8,true,1,true>",
    "moka_wgrad_kernel<32,8,false,1,false>", "moka_wgrad_kernel<32,8,false,1,true>",
    "moka_wgrad_kernel<32,8,true,1,false>", "moka_wgrad_kernel<32,8,true,1,true>",
    "moka_wgrad_wide_kernel<false,false>", "moka_wgrad_wide_kernel<false,true>", "moka_wgrad_wide_kernel<true,false>", "moka_wgrad_wide_kernel<true,true>",
    # down-projection
    "moka_xa_kernel<1,2>", "moka_xa_kernel<1,4>", "moka_xa_kernel<2,4>", "moka_xa_kernel<3,8>",
    "moka_xs_kernel<1>", "moka_xs_kernel<2>", "moka_xs_kernel<3>",
    "moka_xwm_kernel<32,false,1>", "moka_xwm_kernel<32,false,2>", "moka_xwm_kernel<32,false,3>",
    "moka_xwm_kernel<64,false,1>", "moka_xwm_kernel<64,false,2>", "moka_xwm_kernel<64,false,3>", "moka_xwm_kernel<64,true,1>",
}
