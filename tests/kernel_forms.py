"""Every kernel instance in the product library's gfx950 code object, sorted into the two classes of tests/test_gpu_buffer_contract.py:

  PRODUCT           instances a product call selects; the buffer-contract rows reach each of them (a kernel trace of that file
                    lists them all -- see the module docstring there for the command)
  DIAGNOSTICS_ONLY  instances only a moka_tune() override of the diagnostics build selects, or that no launch rule reaches, with the
                    reason

tests/test_kernel_forms_host.py checks that the two sets together are exactly the instances of the built library, so a new form
(a new template instance) must be sorted here -- and, when it is a product form, given a row -- before the suite passes.
Names are demangled, without the argument list and without blanks.
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
    "moka_expand_kernel<16,2,false,2,2,false>", "moka_expand_kernel<16,2,false,3,2,false>",
    "moka_expand_kernel<16,4,false,1,2,false>", "moka_expand_kernel<16,4,true,1,2,false>",
    "moka_expand_kernel<32,4,false,1,2,true>", "moka_expand_kernel<32,4,true,1,2,false>",
    "moka_yt_kernel<16>", "moka_yt_kernel<32>", "moka_yt_kernel<64>",
    "moka_yx_kernel<16>", "moka_yx_kernel<32>", "moka_yx_kernel<64>",
    # fp32 storage
    "moka_f32_expand_kernel<false>", "moka_f32_expand_kernel<true>", "moka_f32_reduce_kernel<false>", "moka_f32_reduce_kernel<true>",
    "moka_f32_wgrad_kernel<false>", "moka_f32_wgrad_kernel<true>",
    # up-projection backward
    "moka_gs_kernel<16,false,false>", "moka_gs_kernel<16,true,false>", "moka_gs_kernel<16,true,true>",
    "moka_gs_kernel<32,false,false>", "moka_gs_kernel<32,true,false>", "moka_gs_kernel<32,true,true>",
    "moka_gy_kernel<16,false,4,false,2>",
    "moka_gy_kernel<16,true,8,false,2>", "moka_gy_kernel<16,true,8,true,2>",
    "moka_gy_kernel<16,true,16,false,2>", "moka_gy_kernel<16,true,16,true,2>",
    # weight gradients
    "moka_wgrad_kernel<16,1,4,false,1,false>", "moka_wgrad_kernel<16,1,4,false,1,true>",
    "moka_wgrad_kernel<16,1,4,false,2,false>", "moka_wgrad_kernel<16,1,4,false,2,true>",
    "moka_wgrad_kernel<16,1,4,false,3,false>", "moka_wgrad_kernel<16,1,4,false,3,true>",
    "moka_wgrad_kernel<16,1,8,false,1,false>", "moka_wgrad_kernel<16,1,8,false,1,true>",
    "moka_wgrad_kernel<16,1,8,true,1,false>", "moka_wgrad_kernel<16,1,8,true,1,true>",
    "moka_wgrad_kernel<32,1,8,false,1,false>", "moka_wgrad_kernel<32,1,8,false,1,true>",
    "moka_wgrad_kernel<32,1,8,true,1,false>", "moka_wgrad_kernel<32,1,8,true,1,true>",
    "moka_wgrad_wide_kernel<false,false>", "moka_wgrad_wide_kernel<false,true>", "moka_wgrad_wide_kernel<true,false>", "moka_wgrad_wide_kernel<true,true>",
    # down-projection
    "moka_xa_kernel<16,1,2>", "moka_xa_kernel<16,1,4>", "moka_xa_kernel<16,2,4>", "moka_xa_kernel<16,3,8>",
    "moka_xs_kernel<1,2,1>", "moka_xs_kernel<2,2,1>", "moka_xs_kernel<3,2,1>",
    "moka_xwm_kernel<32,false,1>", "moka_xwm_kernel<32,false,2>", "moka_xwm_kernel<32,false,3>",
    "moka_xwm_kernel<64,false,1>", "moka_xwm_kernel<64,false,2>", "moka_xwm_kernel<64,false,3>", "moka_xwm_kernel<64,true,1>",
}

_G32_DX3 = 'moka_tune("g32_dx", 3): the first token-owning dx form of groups at rank pads 32 / 64 (k_expand.hip:1378)'
_XA_NG = 'moka_tune("xa_ng", n): groups per workgroup of moka_xa_kernel; the product picks 8 for G = 3, 2 for G = 1 and C > 8192, else 4 (k_reduce.hip:1220)'
_XA_FORM = 'moka_tune("xa_form", 1 / 2): rank pads 32 / 64 use the chunk-walk moka_xwm_kernel unless the form is forced (moka_host.h:145, k_reduce.hip:1264)'
_XW = 'moka_tune("xa_form", 2 / 3) or ("g32_fwd", 1): the staged-weight down-projection (moka_host.h:145, k_reduce.hip:1254-1256)'
_NQ = 'moka_tune("expand_nq", 2 / 3 / 4): column-owning A/B forms of the y / dx kernels (k_expand.hip:1343-1357)'
_GY_NG = 'moka_tune("gy_ng", n): without dB the product always takes 4 groups per workgroup (k_reduce.hip:1139)'
_GY_FORM = 'moka_tune("gy_form", 1): the first (register-staged) g form; rank pad 32 always takes moka_gs_kernel (k_reduce.hip:1101)'
_GY_DEAD = ('unreachable: instantiated by the generic tail of launch_gy_rp, which rank pad 64 never reaches -- both branches of '
            'k_reduce.hip:1103-1134 return first')
_GY_4 = ('moka_tune("gy_ng", 4): moka_gy_kernel runs only for Cmax > 8192 and T > 4096 with G > 1, i.e. >= 34 active column blocks x 129 '
         'token groups, so 8 groups per workgroup already give >= 578 workgroups and the product never drops to 4 on a 256-CU gfx950 (k_reduce.hip:1144)')
_WG_NW = 'moka_tune("wgrad_nw", 4): dB (OUT_CK) always takes the 8-wave form (k_wgrad.hip:575)'
_WG_CT = 'moka_tune("wgrad_ct", 2): two 64-column sub-blocks per wave (k_wgrad.hip:574)'
_G32_DA = 'moka_tune("g32_da", 2): rank pad 32 groups as wave sets on one x tile; the product runs them as a z-batch (moka_api.hip:653)'

DIAGNOSTICS_ONLY = {
    "moka_dxg_kernel<32,2>": _G32_DX3, "moka_dxg_kernel<32,3>": _G32_DX3, "moka_dxg_kernel<64,2>": _G32_DX3, "moka_dxg_kernel<64,3>": _G32_DX3,
    "moka_dxgt_kernel<16,2>": 'moka_tune("g32_dx", 4): the token-owning dx form at rank pad 16 (k_expand.hip:1390)',
    "moka_dxgt_kernel<16,3>": 'moka_tune("g32_dx", 4): the token-owning dx form at rank pad 16 (k_expand.hip:1390)',
    "moka_expand_kernel<16,4,false,1,3,false>": 'moka_tune("expand_depth", 3): three tiles in flight (k_expand.hip:1340)',
    "moka_expand_kernel<16,4,true,1,3,false>": 'moka_tune("expand_depth", 3): three tiles in flight (k_expand.hip:1340)',
    "moka_expand_kernel<32,2,false,1,2,false>": _NQ, "moka_expand_kernel<32,2,true,1,2,false>": _NQ,
    "moka_expand_kernel<64,2,false,1,2,false>": _NQ, "moka_expand_kernel<64,2,true,1,2,false>": _NQ,
    "moka_expand_kernel<64,4,false,1,2,true>": _NQ, "moka_expand_kernel<64,4,true,1,2,false>": _NQ,
    "moka_gy_kernel<16,false,8,false,2>": _GY_NG, "moka_gy_kernel<16,false,16,false,2>": _GY_NG,
    "moka_gy_kernel<16,true,4,false,2>": _GY_4, "moka_gy_kernel<16,true,4,true,2>": _GY_4,
    "moka_gy_kernel<32,false,4,false,2>": _GY_FORM, "moka_gy_kernel<32,false,8,false,2>": _GY_FORM, "moka_gy_kernel<32,false,16,false,2>": _GY_FORM,
    "moka_gy_kernel<64,false,2,false,4>": _GY_FORM, "moka_gy_kernel<64,false,4,false,4>": _GY_FORM,
    "moka_gy_kernel<64,false,4,false,2>": _GY_DEAD, "moka_gy_kernel<64,false,8,false,2>": _GY_DEAD, "moka_gy_kernel<64,false,16,false,2>": _GY_DEAD,
    "moka_wgrad_kernel<16,1,4,true,1,false>": _WG_NW, "moka_wgrad_kernel<16,1,4,true,1,true>": _WG_NW,
    "moka_wgrad_kernel<16,2,8,false,1,false>": _WG_CT, "moka_wgrad_kernel<16,2,8,false,1,true>": _WG_CT,
    "moka_wgrad_kernel<16,2,8,true,1,false>": _WG_CT, "moka_wgrad_kernel<16,2,8,true,1,true>": _WG_CT,
    "moka_wgrad_kernel<32,1,2,false,3,false>": _G32_DA, "moka_wgrad_kernel<32,1,2,false,3,true>": _G32_DA,
    "moka_wgrad_kernel<32,1,4,false,2,false>": _G32_DA, "moka_wgrad_kernel<32,1,4,false,2,true>": _G32_DA,
    "moka_xa_kernel<16,1,8>": _XA_NG, "moka_xa_kernel<16,2,2>": _XA_NG, "moka_xa_kernel<16,2,8>": _XA_NG,
    "moka_xa_kernel<16,3,2>": _XA_NG, "moka_xa_kernel<16,3,4>": _XA_NG,
    "moka_xa_kernel<32,1,2>": _XA_FORM, "moka_xa_kernel<32,1,4>": _XA_FORM, "moka_xa_kernel<32,1,8>": _XA_FORM,
    "moka_xa_kernel<64,1,2>": _XA_FORM, "moka_xa_kernel<64,1,4>": _XA_FORM, "moka_xa_kernel<64,1,8>": _XA_FORM,
    "moka_xs_kernel<1,2,2>": 'moka_tune("xs_wide", 2): 1024-column slices for a single projection (moka_host.h:152)',
    "moka_xw_kernel<16,1,512>": _XW, "moka_xw_kernel<16,2,512>": _XW, "moka_xw_kernel<16,3,512>": _XW,
    "moka_xw_kernel<32,1,512>": _XW, "moka_xw_kernel<64,1,256>": _XW,
}
