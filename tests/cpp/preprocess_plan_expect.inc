// the launches of the commit before the planner, for the rows of preprocess_plan_table.cpp in their order (see its header)
static const char* const EXPECT[] = {
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 0: rgbd vga, n 1
    "k_phase<1,5> 0 4515 1695,2250,570,0/113,150,38,0; k_phase<2,5> 0 2130 570,435,1125,0/38,29,75,0; k_phase<3,5> 0 2460 285,285,1440,450/19,19,1,1; k_phase<4,5> 0 1515 75,1440,0,0/5,1,0,0; k_lm_fast<8,40> 0 450; ",   // 1: rgbd vga, n 15
    "k_blur_mx_pyr 96 368; k_dnormal 0 2400; k_bsplit<1,16> 0 144 80,64,0,0/5,4,0,0; k_dmedian<16> 0 160; k_cgrad<8> 0 48; k_bsplit<2,16> 0 672 96,96,480,0/6,6,1,0; k_lm_fast<8,40> 0 480; ",   // 2: rgbd vga, n 16
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 3: rgbd vga, n 24
    "k_blur_mx_pyr 96 2208; k_dnormal 0 14400; k_bsplit<1,16> 0 864 480,384,0,0/5,4,0,0; k_dmedian<16> 0 960; k_cgrad<8> 0 288; k_bsplit<2,16> 0 4032 576,576,2880,0/6,6,1,0; k_lm_fast<8,40> 0 2880; ",   // 4: rgbd vga, n 96
    "k_blur_mx_pyr 96 368; k_cblur_mx 96 96; k_cgrad_levels<8,8> 0 208; k_dnormal 0 2400; k_dmedian<16> 0 160; k_lm_spread5 0 96; k_lm_spread5 0 96; k_lm_fast<8,40> 0 480; k_lm_fast<8,40> 0 480; ",   // 5: rgbd vga, BATCH_PHASES x busy lanes, n 16
    "k_blur_mx_pyr 96 368; k_cblur_mx 96 96; k_cgrad_levels<8,8> 0 208; k_dnormal 0 2400; k_dmedian<16> 0 160; k_lm_spread5 0 96; k_lm_spread5 0 96; k_lm_fast<8,40> 0 480; k_lm_fast<8,40> 0 480; ",   // 6: rgbd vga, BATCH_PHASES x busy lanes, n 16
    "k_blur_mx_pyr 96 368; k_dnormal 0 2400; k_bsplit<1,16> 0 144 80,64,0,0/5,4,0,0; k_dmedian<16> 0 160; k_cgrad<8> 0 48; k_bsplit<2,16> 0 672 96,96,480,0/6,6,1,0; k_lm_fast<8,40> 0 480; ",   // 7: rgbd vga, BATCH_PHASES x busy lanes, n 16
    "k_blur_mx_pyr 96 368; k_dnormal 0 2400; k_bsplit<1,16> 0 144 80,64,0,0/5,4,0,0; k_dmedian<16> 0 160; k_cgrad<8> 0 48; k_bsplit<2,16> 0 672 96,96,480,0/6,6,1,0; k_lm_fast<8,40> 0 480; ",   // 8: rgbd vga, BATCH_PHASES x busy lanes, n 16
    "k_blur_mx_pyr 96 368; k_dnormal 0 2400; k_bsplit<1,16> 0 144 80,64,0,0/5,4,0,0; k_dmedian<16> 0 160; k_cgrad<8> 0 48; k_bsplit<2,16> 0 672 96,96,480,0/6,6,1,0; k_lm_fast<8,40> 0 480; ",   // 9: rgbd vga, BATCH_PHASES x busy lanes, n 16
    "k_blur_mx_pyr 96 368; k_cblur_mx 96 96; k_cgrad_levels<8,8> 0 208; k_dnormal 0 2400; k_dmedian<16> 0 160; k_lm_spread5 0 96; k_lm_spread5 0 96; k_lm_fast<8,40> 0 480; k_lm_fast<8,40> 0 480; ",   // 10: rgbd vga, BATCH_PHASES x busy lanes, n 16
    "k_blur_mx_pyr 96 2208; k_dnormal 0 14400; k_bsplit<1,16> 0 864 480,384,0,0/5,4,0,0; k_dmedian<16> 0 960; k_cgrad<8> 0 288; k_bsplit<2,16> 0 4032 576,576,2880,0/6,6,1,0; k_lm_fast<8,40> 0 2880; ",   // 11: rgbd vga 96, busy lanes, n 96
    "k_blur_mx_pyr 96 2208; k_cblur_mx 96 576; k_cgrad_levels<16,8> 0 768; k_dnormal 0 14400; k_dmedian<16> 0 960; k_lm_spread5 0 576; k_lm_spread5 0 576; k_lm_fast<8,40> 0 2880; k_lm_fast<8,40> 0 2880; ",   // 12: rgbd vga 96, busy lanes, n 96
    "k_blur_mx_pyr 96 2208; k_cgrad<16> 0 480; k_dnormal 0 14400; k_dmedian<16> 0 960; k_cblur_mx 96 576; k_cgrad<8> 0 288; k_lm_spread5 0 576; k_lm_spread5 0 576; k_lm_fast<8,40> 0 2880; k_lm_fast<8,40> 0 2880; ",   // 13: CGRAD_LEVELS, n 96
    "k_blur_mx_pyr 96 2208; k_cblur_mx 96 576; k_cgrad_levels<16,8> 0 768; k_dnormal 0 14400; k_dmedian<16> 0 960; k_lm_spread5 0 576; k_lm_spread5 0 576; k_lm_fast<8,40> 0 2880; k_lm_fast<8,40> 0 2880; ",   // 14: CGRAD_LEVELS, n 96
    "k_cblur_mx 96 480; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_pyrdown16 0 72; k_cblur_mx 96 144; k_cgrad<8> 0 72; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 15: BLUR_PYR x BLUR_STRIP, n 24
    "k_cblur_mx 16 2880; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_pyrdown16 0 72; k_cblur_mx 16 720; k_cgrad<8> 0 72; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 16: BLUR_PYR x BLUR_STRIP, n 24
    "k_cblur_mx 32 1440; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_pyrdown16 0 72; k_cblur_mx 32 384; k_cgrad<8> 0 72; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 17: BLUR_PYR x BLUR_STRIP, n 24
    "k_cblur_mx 64 768; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_pyrdown16 0 72; k_cblur_mx 64 192; k_cgrad<8> 0 72; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 18: BLUR_PYR x BLUR_STRIP, n 24
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 19: BLUR_PYR x BLUR_STRIP, n 24
    "k_blur_mx_pyr 16 2952; k_cblur_mx 16 720; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 20: BLUR_PYR x BLUR_STRIP, n 24
    "k_blur_mx_pyr 32 1512; k_cblur_mx 32 384; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 21: BLUR_PYR x BLUR_STRIP, n 24
    "k_blur_mx_pyr 64 840; k_cblur_mx 64 192; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 22: BLUR_PYR x BLUR_STRIP, n 24
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 23: BLUR_PYR x BLUR_STRIP, n 24
    "k_blur_mx_pyr 16 2952; k_cblur_mx 16 720; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 24: BLUR_PYR x BLUR_STRIP, n 24
    "k_blur_mx_pyr 32 1512; k_cblur_mx 32 384; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 25: BLUR_PYR x BLUR_STRIP, n 24
    "k_blur_mx_pyr 64 840; k_cblur_mx 64 192; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 26: BLUR_PYR x BLUR_STRIP, n 24
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 27: BLUR_PYR x BLUR_STRIP, n 24
    "k_blur_mx_pyr 16 2952; k_cblur_mx 16 720; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 28: BLUR_PYR x BLUR_STRIP, n 24
    "k_blur_mx_pyr 32 1512; k_cblur_mx 32 384; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 29: BLUR_PYR x BLUR_STRIP, n 24
    "k_blur_mx_pyr 64 840; k_cblur_mx 64 192; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 30: BLUR_PYR x BLUR_STRIP, n 24
    "k_bsplit<0,16> 0 3672 3600,72,0,0/150,3,0,0; k_cblur_sh<16> 0 360; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 31: BLUR_PYR x BLUR_STRIP, fused, n 24
    "k_bsplit<0,16> 0 3672 3600,72,0,0/150,3,0,0; k_cblur_sh<16> 0 360; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 32: BLUR_PYR x BLUR_STRIP, fused, n 24
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 33: BLUR_PYR x BLUR_STRIP, fused, n 24
    "k_blur_mx_pyr 32 1512; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 34: BLUR_PYR x BLUR_STRIP, fused, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 35: CBLUR_VARIANT, n 1
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 36: CBLUR_VARIANT, n 1
    "k_bsplit<0,16> 0 3672 3600,72,0,0/150,3,0,0; k_cblur_sh<16> 0 360; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 37: CBLUR_VARIANT, n 24
    "k_cblur 0 2712; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_pyrdown16 0 72; k_cblur 0 696; k_cgrad<8> 0 72; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 38: CBLUR_VARIANT, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 39: CBLUR_VARIANT, n 1
    "k_cblur_sh<16> 0 15; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur_sh<16> 0 4; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 40: CBLUR_VARIANT, n 1
    "k_blur_pyr<16> 0 432; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 41: CBLUR_VARIANT, n 24
    "k_blur_pyr<16> 0 432; k_cblur_sh<16> 0 96; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 42: CBLUR_VARIANT, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 43: CBLUR_VARIANT, n 1
    "k_cblur_mx 96 20; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur_mx 96 6; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 44: CBLUR_VARIANT, n 1
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 45: CBLUR_VARIANT, n 24
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 46: CBLUR_VARIANT, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 47: CGRAD_VARIANT, n 1
    "k_blur_mx_pyr 96 552; k_corient 0 1800; k_cvote 0 456; k_dnormal 0 3600; k_dmedian<16> 0 240; k_cblur_mx 96 144; k_corient 0 456; k_cvote 0 120; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 48: CGRAD_VARIANT, n 24
    "k_cblur 0 113; k_cgrad<8> 0 10; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_cgrad<8> 0 3; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 49: CGRAD_VARIANT, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 50: CGRAD_VARIANT, n 24
    "k_cblur 0 113; k_cgrad<32> 0 3; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_cgrad<32> 0 1; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 51: CGRAD_VARIANT, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<32,8> 0 144; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 52: CGRAD_VARIANT, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 53: PYRDOWN_VARIANT, n 1
    "k_cblur_mx 96 480; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_pyrdown8 0 912; k_cblur_mx 96 144; k_cgrad<8> 0 72; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 54: PYRDOWN_VARIANT, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown16 0 3; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 55: PYRDOWN_VARIANT, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 56: PYRDOWN_VARIANT, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 57: DMEDIAN_VARIANT, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<4> 0 912; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 58: DMEDIAN_VARIANT, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<16> 0 10; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 59: DMEDIAN_VARIANT, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 60: DMEDIAN_VARIANT, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 61: PHASE_MAX_SLOTS 0, n 1
    "k_blur_mx_pyr 96 368; k_dnormal 0 2400; k_bsplit<1,16> 0 144 80,64,0,0/5,4,0,0; k_dmedian<16> 0 160; k_cgrad<8> 0 48; k_bsplit<2,16> 0 672 96,96,480,0/6,6,1,0; k_lm_fast<8,40> 0 480; ",   // 62: PHASE_MAX_SLOTS 0, n 16
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; mask_rules 0 0; match_masks 0 0; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 63: a masked slot, n 1
    "k_blur_mx_pyr 96 368; k_cblur_mx 96 96; k_cgrad_levels<8,8> 0 208; k_dnormal 0 2400; k_dmedian<16> 0 160; mask_rules 0 0; match_masks 0 0; k_lm_spread5 0 96; k_lm_spread5 0 96; k_lm_fast<8,40> 0 480; k_lm_fast<8,40> 0 480; ",   // 64: a masked slot, n 16
    "k_blur_mx_pyr 96 2208; k_cblur_mx 96 576; k_cgrad_levels<16,8> 0 768; k_dnormal 0 14400; k_dmedian<16> 0 960; mask_rules 0 0; match_masks 0 0; k_lm_spread5 0 576; k_lm_spread5 0 576; k_lm_fast<8,40> 0 2880; k_lm_fast<8,40> 0 2880; ",   // 65: a masked slot, n 96
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 66: planes, n 1
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 67: planes, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 68: planes, n 1
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 69: planes, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 70: planes, n 1
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 71: planes, n 24
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 72: ori_stride % 8, n 24
    "k_phase<1,5> 0 151 113,0,38,0/113,150,38,0; k_phase<2,5> 0 104 0,29,75,0/38,29,75,0; k_phase<3,5> 0 38 19,19,0,0/19,19,19,1; k_phase<4,2> 0 24 5,19,0,0/5,19,0,0; k_lm_fast<8,40> 0 30; ",   // 73: colour vga, n 1
    "k_phase<1,5> 0 2265 1695,0,570,0/113,150,38,0; k_phase<2,5> 0 1560 0,435,1125,0/38,29,75,0; k_phase<3,5> 0 570 285,285,0,0/19,19,19,1; k_phase<4,2> 0 360 75,285,0,0/5,19,0,0; k_lm_fast<8,40> 0 450; ",   // 74: colour vga, n 15
    "k_blur_mx_pyr 96 368; k_bphase<2,2,16,16> 0 144 80,0,64,0/5,10,4,0; k_bphase<3,2,16,16> 0 336 32,304,0,0/2,19,19,1; k_lm_fast<8,40> 0 480; ",   // 75: colour vga, n 16
    "k_blur_mx_pyr 96 2208; k_bphase<2,2,16,16> 0 864 480,0,384,0/5,10,4,0; k_bphase<3,2,16,16> 0 2016 192,1824,0,0/2,19,19,1; k_lm_fast<8,40> 0 2880; ",   // 76: colour vga, n 96
    "k_blur_mx_pyr 96 2208; k_cblur_mx 96 576; k_cgrad_levels<16,8> 0 768; k_lm_spread2 0 1824; k_lm_fast<8,40> 0 2880; ",   // 77: colour vga, busy lanes, n 96
    "k_blur_mx_pyr 96 552; k_bphase<2,5,16,16> 0 216 120,0,96,0/5,10,4,0; k_bphase<3,5,16,16> 0 192 48,144,0,0/2,6,6,1; k_lm_fast<8,40> 0 720; ",   // 78: colour vga, T {5, 8}, n 24
    "k_phase<1,5> 0 151 113,0,38,0/113,150,38,0; k_phase<2,5> 0 104 0,29,75,0/38,29,75,0; k_phase<3,5> 0 38 19,19,0,0/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 79: colour vga, T {5, 8}, n 1
    "k_phase<1,5> 0 600 450,0,150,0/450,600,150,0; k_phase<2,5> 0 413 0,113,300,0/150,113,300,0; k_phase<3,5> 0 150 75,75,0,0/75,75,75,2; k_phase<4,2> 0 94 19,75,0,0/19,75,0,0; k_lm_fast<8,40> 0 120; ",   // 80: colour 1280 x 960, WORK_WEIGHT, n 1
    "k_phase<1,5> 0 1800 1350,0,450,0/450,600,150,0; k_phase<2,5> 0 1239 0,339,900,0/150,113,300,0; k_phase<3,5> 0 450 225,225,0,0/75,75,75,2; k_phase<4,2> 0 282 57,225,0,0/19,75,0,0; k_lm_fast<8,40> 0 360; ",   // 81: colour 1280 x 960, WORK_WEIGHT, n 3
    "k_blur_pyr<16> 0 276; k_bphase<2,2,32,32> 0 100 40,0,60,0/10,38,15,0; k_bphase<3,2,32,32> 0 320 20,300,0,0/5,75,75,2; k_lm_fast<8,80> 0 240; ",   // 82: colour 1280 x 960, WORK_WEIGHT, n 4
    "k_blur_pyr<16> 0 552; k_bphase<2,2,32,32> 0 200 80,0,120,0/10,38,15,0; k_bphase<3,2,32,32> 0 640 40,600,0,0/5,75,75,2; k_lm_fast<8,80> 0 480; ",   // 83: colour 1280 x 960, WORK_WEIGHT, n 8
    "k_phase<1,5> 0 600 450,0,150,0/450,600,150,0; k_phase<2,5> 0 413 0,113,300,0/150,113,300,0; k_phase<3,5> 0 150 75,75,0,0/75,75,75,2; k_phase<4,2> 0 94 19,75,0,0/19,75,0,0; k_lm_fast<8,40> 0 120; ",   // 84: colour 1280 x 960, WORK_WEIGHT, n 1
    "k_phase<1,5> 0 1800 1350,0,450,0/450,600,150,0; k_phase<2,5> 0 1239 0,339,900,0/150,113,300,0; k_phase<3,5> 0 450 225,225,0,0/75,75,75,2; k_phase<4,2> 0 282 57,225,0,0/19,75,0,0; k_lm_fast<8,40> 0 360; ",   // 85: colour 1280 x 960, WORK_WEIGHT, n 3
    "k_phase<1,5> 0 2400 1800,0,600,0/450,600,150,0; k_phase<2,5> 0 1652 0,452,1200,0/150,113,300,0; k_phase<3,5> 0 600 300,300,0,0/75,75,75,2; k_phase<4,2> 0 376 76,300,0,0/19,75,0,0; k_lm_fast<8,40> 0 480; ",   // 86: colour 1280 x 960, WORK_WEIGHT, n 4
    "k_phase<1,5> 0 4800 3600,0,1200,0/450,600,150,0; k_phase<2,5> 0 3304 0,904,2400,0/150,113,300,0; k_phase<3,5> 0 1200 600,600,0,0/75,75,75,2; k_phase<4,2> 0 752 152,600,0,0/19,75,0,0; k_lm_fast<8,40> 0 960; ",   // 87: colour 1280 x 960, WORK_WEIGHT, n 8
    "k_blur_pyr<16> 0 276; k_cblur_mx 96 80; k_cgrad_levels<8,8> 0 196; k_lm_spread2 0 300; k_lm_fast<8,80> 0 240; ",   // 88: colour 1280 x 960, busy lanes, n 4
    "k_blur_pyr<16> 0 552; k_cblur_mx 96 160; k_cgrad_levels<8,8> 0 392; k_lm_spread2 0 600; k_lm_fast<8,80> 0 480; ",   // 89: colour 1280 x 960, busy lanes, n 8
    "k_blur_pyr<32> 0 1280; k_cblur_mx 96 640; k_cgrad_levels<16,8> 0 960; k_lm_spread2 0 2400; k_lm_fast<8,80> 0 1920; ",   // 90: colour 1280 x 960, busy lanes, n 32
    "k_bphase<1,2,32,32> 0 320 0,240,80,0/600,30,10,0; k_bphase<2,2,32,32> 0 200 80,0,120,0/10,38,15,0; k_bphase<3,2,32,32> 0 640 40,600,0,0/5,75,75,2; k_lm_fast<8,80> 0 480; ",   // 91: colour 1280 x 960, BLUR_PYR 0, n 8
    "k_bphase<1,2,32,32> 0 1280 0,960,320,0/600,30,10,0; k_bphase<2,2,32,32> 0 800 320,0,480,0/10,38,15,0; k_bphase<3,2,32,32> 0 2560 160,2400,0,0/5,75,75,2; k_lm_fast<8,80> 0 1920; ",   // 92: colour 1280 x 960, BLUR_PYR 0, n 32
    "k_phase<1,5> 0 2400 900,1200,300,0/450,600,150,0; k_phase<2,5> 0 1126 300,226,600,0/150,113,300,0; k_phase<3,5> 0 1308 150,150,768,240/75,75,2,2; k_phase<4,5> 0 806 38,768,0,0/19,2,0,0; k_lm_fast<8,40> 0 240; ",   // 93: rgbd 1280 x 960, n 2
    "k_blur_pyr<16> 0 552; k_dnormal 0 4800; k_bsplit<1,32> 0 200 80,120,0,0/10,15,0,0; k_dmedian<16> 0 304; k_cgrad<8> 0 80; k_bsplit<2,16> 0 1344 192,192,960,0/24,24,2,0; k_lm_fast<8,80> 0 480; ",   // 94: rgbd 1280 x 960, n 8
    "k_blur_pyr<16> 0 552; k_cblur_mx 96 160; k_cgrad_levels<8,8> 0 392; k_dnormal 0 4800; k_dmedian<16> 0 304; k_lm_spread5 0 192; k_lm_spread5 0 192; k_lm_fast<8,80> 0 480; k_lm_fast<8,80> 0 480; ",   // 95: rgbd 1280 x 960, busy lanes, n 8
    "k_blur_pyr<32> 0 1280; k_cblur_mx 96 640; k_cgrad_levels<16,8> 0 960; k_dnormal 0 19200; k_dmedian<16> 0 1216; k_lm_spread5 0 768; k_lm_spread5 0 768; k_lm_fast<8,80> 0 1920; k_lm_fast<8,80> 0 1920; ",   // 96: rgbd 1280 x 960, busy lanes, n 32
    "k_bsplit<0,16> 0 4880 4800,80,0,0/600,10,0,0; k_cblur_sh<32> 0 240; k_bsplit<1,32> 0 200 80,120,0,0/10,15,0,0; k_dmedian<16> 0 304; k_cgrad<8> 0 80; k_bsplit<2,16> 0 1344 192,192,960,0/24,24,2,0; k_lm_fast<8,80> 0 480; ",   // 97: rgbd 1280 x 960, BLUR_PYR 0, n 8
    "k_blur_mx_pyr 96 168; k_cblur_mx 96 48; k_cgrad_levels<8,8> 0 96; k_dnormal 0 912; k_dmedian<16> 0 72; k_lm_spread5 0 48; k_lm_spread5 0 48; k_lm_fast<8,40> 0 360; k_lm_fast<8,40> 0 360; ",   // 98: rgbd 320 x 240, n 24
    "k_blur_mx_pyr 96 168; k_cblur_mx 96 48; k_cgrad_levels<8,8> 0 96; k_dnormal 0 912; k_dmedian<16> 0 72; k_lm_spread5 0 48; k_lm_spread5 0 48; k_lm_fast<8,40> 0 360; k_lm_fast<8,40> 0 360; ",   // 99: rgbd 320 x 240, n 24
    "k_blur_mx_pyr 96 672; k_cblur_mx 96 192; k_cgrad_levels<8,8> 0 384; k_dnormal 0 3648; k_dmedian<16> 0 288; k_lm_spread5 0 192; k_lm_spread5 0 192; k_lm_fast<8,40> 0 1440; k_lm_fast<8,40> 0 1440; ",   // 100: rgbd 320 x 240, n 96
    "k_blur_mx_pyr 96 672; k_cblur_mx 96 192; k_cgrad_levels<8,8> 0 384; k_dnormal 0 3648; k_dmedian<16> 0 288; k_lm_spread5 0 192; k_lm_spread5 0 192; k_lm_fast<8,40> 0 1440; k_lm_fast<8,40> 0 1440; ",   // 101: rgbd 320 x 240, n 96
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_pyrdown8 0 10; k_cblur 0 8; k_corient 0 5; k_cvote 0 2; k_nn_half 0 5x60x1; k_nn_half 0 3x30x1; k_lm_fast<4,64> 0 360; k_lm_fast<4,64> 0 360; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 15; k_lm_fast<8,40> 0 15; ",   // 102: three levels, n 1
    "k_blur_mx_pyr 96 552; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_cblur_mx 96 144; k_cgrad<8> 0 72; k_pyrdown16 0 24; k_cblur_mx 96 48; k_cgrad<8> 0 24; k_nn_half 0 5x60x24; k_nn_half 0 3x30x24; k_lm_fast<4,64> 0 8640; k_lm_fast<4,64> 0 8640; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 360; k_lm_fast<8,40> 0 360; ",   // 103: three levels, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_pyrdown8 0 10; k_cblur 0 8; k_corient 0 5; k_cvote 0 2; k_pyrdown8 0 3; k_cblur 0 2; k_corient 0 2; k_cvote 0 1; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 15; k_linear_memories 12 1x7x1 +5168; ",   // 104: four levels, colour, n 1
    "k_cblur_mx 96 480; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_fast<8,80> 0 1440; k_lm_fast<8,80> 0 1440; ",   // 105: one level, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_depth_quantize 0 10x60x1; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 106: LUT not one-hot, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_depth_quantize 0 10x60x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 107: LUT not one-hot, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 108: LM_FLAG_BYTE_RESPONSES, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 109: LM_FLAG_BYTE_RESPONSES, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<4,64> 0 360; k_lm_fast<4,64> 0 360; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 110: T {4, 8}, n 1
    "k_blur_mx_pyr 96 336; k_cblur_sh<16> 0 72; k_cgrad_levels<8,8> 0 192; k_dnormal 0 2040; k_dmedian<16> 0 144; k_lm_fast<4,64> 0 4320; k_lm_fast<4,64> 0 4320; k_lm_fast<4,64> 0 1080; k_lm_fast<4,64> 0 1080; ",   // 111: rgbd 480 x 360 (w % 32 != 0), n 24
    "k_color_quantize 0 20x60x1; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown 0 5x60x1; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 112: misaligned, n 1
    "k_color_quantize 0 20x60x24; k_dnormal 0 3600; k_dmedian<16> 0 240; k_pyrdown 0 5x60x24; k_cblur_mx 96 144; k_cgrad<8> 0 72; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 113: misaligned, n 24
    "k_color_quantize 0 20x60x1; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown 0 5x60x1; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 114: misaligned, n 1
    "k_color_quantize 0 20x60x24; k_dnormal 0 3600; k_dmedian<16> 0 240; k_pyrdown 0 5x60x24; k_cblur_mx 96 144; k_cgrad<8> 0 72; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 115: misaligned, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_color_quantize 0 10x30x1; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 116: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_color_quantize 0 10x30x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 117: misaligned, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown 0 5x60x1; k_color_quantize 0 10x30x1; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 118: misaligned, n 1
    "k_cblur_mx 96 480; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_pyrdown 0 5x60x24; k_color_quantize 0 10x30x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 119: misaligned, n 24
    "k_color_quantize 0 20x60x1; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 120: misaligned, n 1
    "k_color_quantize 0 20x60x24; k_dnormal 0 3600; k_dmedian<16> 0 240; k_pyrdown16 0 72; k_cblur_mx 96 144; k_cgrad<8> 0 72; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 121: misaligned, n 24
    "k_color_quantize 0 20x60x1; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 122: misaligned, n 1
    "k_color_quantize 0 20x60x24; k_dnormal 0 3600; k_dmedian<16> 0 240; k_pyrdown16 0 72; k_cblur_mx 96 144; k_cgrad<8> 0 72; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 123: misaligned, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_color_quantize 0 10x30x1; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 124: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_color_quantize 0 10x30x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 125: misaligned, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_color_quantize 0 10x30x1; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 126: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_color_quantize 0 10x30x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 127: misaligned, n 24
    "k_color_quantize 0 20x60x1; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 128: misaligned, n 1
    "k_color_quantize 0 20x60x24; k_dnormal 0 3600; k_dmedian<16> 0 240; k_pyrdown16 0 72; k_cblur_mx 96 144; k_cgrad<8> 0 72; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 129: misaligned, n 24
    "k_color_quantize 0 20x60x1; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 130: misaligned, n 1
    "k_color_quantize 0 20x60x24; k_dnormal 0 3600; k_dmedian<16> 0 240; k_pyrdown16 0 72; k_cblur_mx 96 144; k_cgrad<8> 0 72; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 131: misaligned, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_color_quantize 0 10x30x1; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 132: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_color_quantize 0 10x30x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 133: misaligned, n 24 -- NOT the earlier launches, on purpose (no level-1 blur ahead of the fallback kernel: see the table's header)
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_dnormal 0 150; k_dmedian<4> 0 38; k_pyrdown8 0 38; k_color_quantize 0 10x30x1; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 134: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_color_quantize 0 10x30x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 135: misaligned, n 24 -- NOT the earlier launches, on purpose (no level-1 blur ahead of the fallback kernel: see the table's header)
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 136: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 137: misaligned, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_depth_quantize 0 10x60x1; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 138: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_depth_quantize 0 10x60x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 139: misaligned, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 140: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 141: misaligned, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 142: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_fast<5,128> 0 2304; k_lm_fast<5,128> 0 2304; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 143: misaligned, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 144: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 145: misaligned, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 146: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 147: misaligned, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 148: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 149: misaligned, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 150: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_dnormal 0 3600; k_dmedian<16> 0 240; k_lm_spread5 0 144; k_lm_fast<5,128> 0 2304; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 151: misaligned, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 152: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 153: misaligned, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 154: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 155: misaligned, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_depth_quantize 0 10x60x1; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 156: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_depth_quantize 0 10x60x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 157: misaligned, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_depth_quantize 0 10x60x1; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 158: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_depth_quantize 0 10x60x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 159: misaligned, n 24
    "k_phase<1,5> 0 301 113,150,38,0/113,150,38,0; k_phase<2,5> 0 142 38,29,75,0/38,29,75,0; k_phase<3,5> 0 164 19,19,96,30/19,19,1,1; k_phase<4,5> 0 101 5,96,0,0/5,1,0,0; k_lm_fast<8,40> 0 30; ",   // 160: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_dnormal 0 3600; k_bsplit<1,16> 0 216 120,96,0,0/5,4,0,0; k_dmedian<16> 0 240; k_cgrad<8> 0 72; k_bsplit<2,16> 0 1008 144,144,720,0/6,6,1,0; k_lm_fast<8,40> 0 720; ",   // 161: misaligned, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_depth_quantize 0 10x60x1; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 162: misaligned, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_depth_quantize 0 10x60x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 163: misaligned, n 24
    "k_color_quantize 0 20x60x1; k_depth_quantize 0 10x60x1; k_pyrdown 0 5x60x1; k_color_quantize 0 10x30x1; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 164: misaligned, n 1
    "k_color_quantize 0 20x60x24; k_depth_quantize 0 10x60x24; k_pyrdown 0 5x60x24; k_color_quantize 0 10x30x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 165: misaligned, n 24
    "k_color_quantize 0 20x60x1; k_depth_quantize 0 10x60x1; k_pyrdown 0 5x60x1; k_color_quantize 0 10x30x1; k_lm_fast<5,128> 0 96; k_lm_fast<5,128> 0 96; k_lm_fast<8,40> 0 30; k_lm_fast<8,40> 0 30; ",   // 166: misaligned, n 1
    "k_color_quantize 0 20x60x24; k_depth_quantize 0 10x60x24; k_pyrdown 0 5x60x24; k_color_quantize 0 10x30x24; k_lm_fast<5,128> 0 2304; k_lm_fast<5,128> 0 2304; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 167: misaligned, n 24
    "k_color_quantize 0 20x60x1; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<2,128> 0 720; k_lm_fast<8,40> 0 30; ",   // 168: misaligned, colour, n 1
    "k_color_quantize 0 20x60x24; k_pyrdown16 0 72; k_cblur_mx 96 144; k_cgrad<8> 0 72; k_lm_fast<2,128> 0 17280; k_lm_fast<8,40> 0 720; ",   // 169: misaligned, colour, n 24
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; k_pyrdown8 0 38; k_cblur 0 29; k_corient 0 19; k_cvote 0 5; k_lm_fast<2,128> 0 720; k_lm_fast<8,40> 0 30; ",   // 170: misaligned, colour, n 1
    "k_blur_mx_pyr 96 552; k_cblur_mx 96 144; k_cgrad_levels<8,8> 0 312; k_lm_fast<2,128> 0 17280; k_lm_fast<8,40> 0 720; ",   // 171: misaligned, colour, n 24
    "k_color_quantize 0 20x60x1; k_pyrdown 0 5x60x1; k_color_quantize 0 10x30x1; k_lm_fast<2,128> 0 720; k_lm_fast<8,40> 0 30; ",   // 172: misaligned, colour, n 1
    "k_color_quantize 0 20x60x24; k_pyrdown 0 5x60x24; k_color_quantize 0 10x30x24; k_lm_fast<2,128> 0 17280; k_lm_fast<8,40> 0 720; ",   // 173: misaligned, colour, n 24
    "k_blur_mx_pyr 96 552; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_color_quantize 0 10x30x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 174: misaligned, busy lanes, n 24
    "k_blur_mx_pyr 96 552; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_color_quantize 0 10x30x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 175: misaligned, busy lanes, n 24
    "k_blur_mx_pyr 96 552; k_cgrad<8> 0 240; k_dnormal 0 3600; k_dmedian<16> 0 240; k_color_quantize 0 10x30x24; k_lm_spread5 0 144; k_lm_spread5 0 144; k_lm_fast<8,40> 0 720; k_lm_fast<8,40> 0 720; ",   // 176: misaligned, busy lanes, n 24 -- NOT the earlier launches, on purpose (no level-1 blur ahead of the fallback kernel: see the table's header)
    "k_color_quantize 0 2x7x1; ",   // 177: stage colour, n 1
    "k_color_quantize 0 2x7x1; ",   // 178: stage colour, n 1
    "k_cblur 0 1; k_corient 0 1; k_cvote 0 1; ",   // 179: stage colour, n 1
    "k_cblur 0 1; k_corient 0 1; k_cvote 0 1; ",   // 180: stage colour, n 1
    "k_color_quantize 0 1; ",   // 181: stage colour, n 1
    "k_color_quantize 0 1; ",   // 182: stage colour, n 1
    "k_color_quantize 0 1x10x1; ",   // 183: stage colour, n 1
    "k_color_quantize 0 1x10x1; ",   // 184: stage colour, n 1
    "k_color_quantize 0 1x12x1; ",   // 185: stage colour, n 1
    "k_color_quantize 0 1x12x1; ",   // 186: stage colour, n 1
    "k_color_quantize 0 2; ",   // 187: stage colour, n 1
    "k_color_quantize 0 2; ",   // 188: stage colour, n 1
    "k_cblur 0 2; k_corient 0 1; k_cvote 0 1; ",   // 189: stage colour, n 1
    "k_cblur 0 2; k_corient 0 1; k_cvote 0 1; ",   // 190: stage colour, n 1
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; ",   // 191: stage colour, n 1
    "k_cblur 0 113; k_corient 0 75; k_cvote 0 19; ",   // 192: stage colour, n 1
    "k_cblur 0 450; k_corient 0 300; k_cvote 0 75; ",   // 193: stage colour, n 1
    "k_cblur 0 450; k_corient 0 300; k_cvote 0 75; ",   // 194: stage colour, n 1
    "k_pyrdown 0 1x7x1; ",   // 195: stage pyrDown, n 1
    "k_pyrdown8 0 1; ",   // 196: stage pyrDown, n 1
    "k_pyrdown 0 1; ",   // 197: stage pyrDown, n 1
    "k_pyrdown 0 1x10x1; ",   // 198: stage pyrDown, n 1
    "k_pyrdown 0 1x12x1; ",   // 199: stage pyrDown, n 1
    "k_pyrdown 0 1; ",   // 200: stage pyrDown, n 1
    "k_pyrdown8 0 1; ",   // 201: stage pyrDown, n 1
    "k_pyrdown8 0 38; ",   // 202: stage pyrDown, n 1
    "k_pyrdown8 0 150; ",   // 203: stage pyrDown, n 1
    "k_depth_quantize 0 1x7x1; ",   // 204: stage depth, n 1
    "k_dnormal 0 1; k_dmedian<4> 0 1; ",   // 205: stage depth, n 1
    "k_dnormal 0 1; k_dmedian<4> 0 1; ",   // 206: stage depth, n 1
    "k_depth_quantize 0 1x10x1; ",   // 207: stage depth, n 1
    "k_depth_quantize 0 1x12x1; ",   // 208: stage depth, n 1
    "k_depth_quantize 0 1; ",   // 209: stage depth, n 1
    "k_dnormal 0 2; k_dmedian<4> 0 1; ",   // 210: stage depth, n 1
    "k_dnormal 0 150; k_dmedian<4> 0 38; ",   // 211: stage depth, n 1
    "k_dnormal 0 600; k_dmedian<4> 0 150; ",   // 212: stage depth, n 1
    "k_depth_quantize 0 10x60x1; ",   // 213: stage depth, LUT not one-hot, n 1
    "k_cblur 0 113; k_cgrad<8> 0 10; ",   // 214: stage colour, CGRAD_VARIANT 2, n 1
    "k_cblur_mx 96 20; k_corient 0 75; k_cvote 0 19; ",   // 215: stage colour, CBLUR_VARIANT 4, n 1
    "k_pyrdown16 0 3; ",   // 216: stage pyrDown, PYRDOWN_VARIANT 2, n 1
    "k_lm_fast<2,128> 0 720; ",   // 217: stage linear memories, n 1
    "k_lm_fast<4,64> 0 360; ",   // 218: stage linear memories, n 1
    "k_lm_fast<5,128> 0 96; ",   // 219: stage linear memories, n 1
    "k_lm_fast<8,40> 0 120; ",   // 220: stage linear memories, n 1
    "k_lm_fast<8,40> 0 30; ",   // 221: stage linear memories, n 1
    "k_linear_memories 16 1x12x1 +2568; ",   // 222: stage linear memories, n 1
    "k_lm_fast<5,128> 0 4; ",   // 223: stage linear memories, n 1
    "k_linear_memories 4 1x3x1 +3248; ",   // 224: stage linear memories, n 1
    "k_linear_memories 12 1x5x1 +3808; ",   // 225: stage linear memories, n 1
    "k_linear_memories 12 1x5x1 +4440; ",   // 226: stage linear memories, n 1
    "k_linear_memories 4 3x10x1 +7008; ",   // 227: stage linear memories, n 1
    "k_linear_memories 20 1x18x1 +2312; ",   // 228: stage linear memories, n 1
};
