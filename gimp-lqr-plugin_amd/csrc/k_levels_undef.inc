// k_levels_undef.inc -- drops what a family of the level kernel defined for k_levels_body.inc
#undef LV_NT
#undef LV_SLOT_STATE
#undef LV_POLLED
#undef LV_A
#undef LV_WAVE
#undef LV_BLOCK
#undef LV_INIT_FLAGS
#undef LV_AFTER_SETUP
#undef LV_DBG
#undef LV_STATS
#undef LV_TIME
#undef LV_LEVEL_END
#undef LV_TRACK
